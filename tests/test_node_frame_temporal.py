"""The temporal stage of the frame denoiser driven from JavaScript (WebGPURenderer.frameTemporalDesc / setFrameTemporal /
resetFrameHistory of node/index.js): the addon exports the bindings, and `node render_cornell.js ... --denoise PASSES --temporal
MAX_HISTORY` presents and filters the very words the Python binding gives for the same call sequence."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_util as pu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
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
    js = ("const m=require('%s/index.js');const P=m.WebGPURenderer.prototype;console.log(typeof m.native.rtSetFrameTemporal,"
          "typeof m.native.rtResetFrameHistory,typeof m.WebGPURenderer.frameTemporalDesc,typeof P.setFrameTemporal,"
          "typeof P.resetFrameHistory,Array.from(m.WebGPURenderer.frameTemporalDesc({planeEps:0.5,sameInstance:true,maxHistory:8})).join());"
          "try{m.WebGPURenderer.frameTemporalDesc({})}catch(e){console.log(e.constructor.name)}" % node_dir)
    out = subprocess.run([node, "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 5 + ["1,8,4,0.9,0.5", "TypeError"]
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    for m in ("frameTemporalDesc(", "setFrameTemporal(", "resetFrameHistory("):
        assert m in dts, m
    assert "--temporal" in open(os.path.join(node_dir, "render_cornell.js")).read()


@needs_node
@pytest.mark.gpu
def test_javascript_filtered_frames_match_python(W):
    from webgpu_raytracer_amd import renderer as R
    assert W._build.build_node_addon()
    out = subprocess.run([node, os.path.join(NODE_DIR, "render_cornell.js"), "cornell", "33", "9", "3", "4", "--denoise", "4",
                          "--temporal", "8"], check=True, capture_output=True, text=True, timeout=300).stdout
    js = json.loads(out.strip().splitlines()[-1])
    assert js["denoise"] == 4 and js["temporal"] == 8 and js["planeEps"] == 0.02
    W._build.build_rt()
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    shas = {}
    for temporal in (True, False):
        r = W.WebGPURenderer(0)          # after the child has gone: one context at a time
        try:
            r.buildPipeline(4, 1)
            W.upload_scene(r, pu.bridge_for(W, "cornell"), 33, 9)
            d = R.frame_denoise_desc(4, plane_eps=0.02)
            r.setPresentDenoise(d)
            if temporal:
                r.setFrameTemporal(R.frame_temporal_desc(8, plane_eps=0.02))
            for f in (1, 2, 3):
                r.compute(f)
                r.present()
            shas[temporal] = (sha(r.captureFrame()["data"]), sha(r.readAccum()), sha(r.denoiseFrame(d)))
            if temporal:
                assert r.readFrameHistory(frames_only=True) == 3
        finally:
            r.destroy()
    assert (js["rgba_sha256"], js["accum_sha256"], js["denoised_sha256"]) == shas[True]
    assert shas[True][2] != shas[False][2] and shas[True][1] == shas[False][1]   # the stage changes the filtered frame alone
