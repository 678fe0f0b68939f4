"""Frame motion driven from JavaScript (frameTemporalDesc({motion}), setFrameMotionIds, readFrameMotion of node/index.js): the
addon exports the bindings, the descriptor carries the flag, and node/animate_glb.js takes --denoise / --temporal / --motion."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")


@needs_node
def test_node_addon_exports_the_bindings(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');const P=m.WebGPURenderer.prototype;const D=m.WebGPURenderer.frameTemporalDesc;"
          "console.log(typeof m.native.rtSetFrameMotionIds,typeof m.native.rtReadFrameMotion,typeof P.setFrameMotionIds,"
          "typeof P.readFrameMotion,Array.from(D({planeEps:0.5,motion:true})).join(),"
          "Array.from(D({planeEps:0.5,motion:true,sameInstance:true,maxHistory:8})).join(),Array.from(D({planeEps:0.5})).join());"
          % node_dir)
    out = subprocess.run([node, "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 4 + ["2,32,4,0.9,0.5", "3,8,4,0.9,0.5", "0,32,4,0.9,0.5"]
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    for m in ("motion?: boolean", "setFrameMotionIds(", "readFrameMotion("):
        assert m in dts, m
    src = open(os.path.join(node_dir, "animate_glb.js")).read()
    for flag in ("--denoise", "--temporal", "--motion"):
        assert flag in src, flag


@needs_node
@pytest.mark.gpu
def test_animate_glb_follows_the_skinned_mesh(W, tmp_path):
    import json
    import test_gltf
    assert W._build.build_node_addon()
    glb = tmp_path / "skinned.glb"
    glb.write_bytes(test_gltf.build_skinned(W)[0].glb())
    env = dict(os.environ, RT_NODE_DEVICE_UPDATE="1")
    runs = {}
    for flags in (("--motion",), ()):
        out = subprocess.run([node, os.path.join(REPO, "webgpu-raytracer_amd", "node", "animate_glb.js"), str(glb), "70", "37", "4", "1",
                              "4", "--denoise", "2", "--temporal", "8"] + list(flags), check=True, capture_output=True, text=True,
                             timeout=300, env=env).stdout
        runs[flags] = json.loads(out.strip().splitlines()[-1])
    m, s = runs[("--motion",)], runs[()]
    assert m["deviceResident"] and m["motion"] is True and m["temporal"] == 8 and m["denoise"] == 2
    assert m["moved"] > 0, "the animated strip is in view and moves every frame"
    assert m["accum_sha256"] == s["accum_sha256"], "the stage changes the filtered frame alone"
    assert "motion" not in s
