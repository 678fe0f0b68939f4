"""The sharded image from the Node host: the addon binds rt_dist_*, index.js / index.d.ts carry the methods, and
node/render_sharded.js renders one image as several ranks - bit for bit what render_cornell.js renders on one context and
what the CPU oracle computes.  Every child process has a time limit and is killed when it expires."""
import hashlib
import json
import os
import re
import shutil
import signal
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
METHODS = ("setStripes", "distInit", "distShutdown", "distBlockBytes", "packStripes", "readBlock", "writeBlock",
           "unpackStripes", "gatherStripes", "readDisplay", "distUniqueId")
NATIVE = ("rtSetStripes", "rtDistUniqueId", "rtDistInit", "rtDistShutdown", "rtDistBlockBytes", "rtPackStripes",
          "rtDistReadBlock", "rtDistWriteBlock", "rtUnpackStripes", "rtGatherStripes", "rtReadDisplay", "rtDeviceCount")

node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"),
                                reason="node / node_api.h not present")


@pytest.fixture(scope="module")
def addon(W):
    W._build.build_rt()
    path = W._build.build_node_addon()
    assert path and os.path.exists(path)
    return path


def run_json(args, env=None, timeout=300):
    """node <args> in a process group of its own, so that on expiry the forked ranks are killed with their parent."""
    p = subprocess.Popen([node] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, start_new_session=True)
    try:
        stdout, stderr = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        stdout, stderr = p.communicate()
        pytest.fail("node %s did not finish within %d s and was killed\n%s" % (" ".join(args[:1]), timeout, (stdout + stderr)[-3000:]))
    assert p.returncode == 0, (stdout + stderr)[-3000:]
    return json.loads(stdout.strip().splitlines()[-1])


def test_typings_and_class_declare_the_sharded_methods():
    dts = open(os.path.join(NODE_DIR, "index.d.ts")).read()
    js = open(os.path.join(NODE_DIR, "index.js")).read()
    for m in METHODS:
        assert re.search(r"\b%s\(" % m, dts), "index.d.ts does not declare %s" % m
        assert re.search(r"^\s+(static\s+)?%s\(" % m, js, re.M), "index.js has no method %s" % m
    assert os.path.exists(os.path.join(NODE_DIR, "render_sharded.js"))


@needs_node
def test_addon_exports_the_sharded_calls(W, addon):
    js = ("const {native,WebGPURenderer}=require('%s/index.js');const o={};for(const n of %s)o[n]=typeof native[n];"
          "for(const m of %s)o['m_'+m]=typeof (WebGPURenderer.prototype[m]||WebGPURenderer[m]);console.log(JSON.stringify(o));"
          % (NODE_DIR, json.dumps(list(NATIVE)), json.dumps(list(METHODS))))
    got = run_json(["-e", js], timeout=120)
    assert got == dict([(n, "function") for n in NATIVE] + [("m_" + m, "function") for m in METHODS])


def _assert_matches_one_context_and_oracle(W, oracle_lib, got):
    one = run_json([os.path.join(NODE_DIR, "render_cornell.js"), "cornell", "96", "80", "7", "4"])
    b = W.WorldBridge()
    b.loadScene("cornell")
    cpu = oracle_lib.OracleRenderer()
    cpu.buildPipeline(4, 1)
    W.upload_scene(cpu, b, 96, 80)
    for f in range(1, 8):
        cpu.compute(f)
        cpu.present()
    assert got["accum_sha256"] == one["accum_sha256"] == hashlib.sha256(cpu.readAccum().tobytes()).hexdigest()
    assert got["rgba_sha256"] == one["rgba_sha256"] == hashlib.sha256(cpu.captureFrame()["data"].tobytes()).hexdigest()
    assert got["counters"] == one["counters"]
    c = cpu.getCounters()
    for k in ("primary_rays", "extension_rays", "shadow_rays"):
        assert got["counters"][k] == c[k]


@needs_node
@pytest.mark.gpu
def test_two_contexts_as_ranks_from_javascript_match_one_context_and_the_oracle(W, oracle_lib, addon):
    """`render_sharded.js cornell 96 80 7 4 2` with the ranks as contexts of one process, blocks through readBlock / writeBlock."""
    env = dict(os.environ, RT_NODE_SHARDED_MODE="contexts")
    got = run_json([os.path.join(NODE_DIR, "render_sharded.js"), "cornell", "96", "80", "7", "4", "2"], env=env)
    assert got["mode"] == "contexts" and got["world"] == 2
    _assert_matches_one_context_and_oracle(W, oracle_lib, got)


@needs_node
@pytest.mark.gpu
def test_default_mode_on_this_machine_matches_too(W, oracle_lib, addon):
    """No mode forced: contexts on a one-GPU machine, forked RCCL ranks where there are two GPUs."""
    from webgpu_raytracer_amd import renderer
    env = {k: v for k, v in os.environ.items() if k != "RT_NODE_SHARDED_MODE"}
    got = run_json([os.path.join(NODE_DIR, "render_sharded.js"), "cornell", "96", "80", "7", "4", "2"], env=env, timeout=400)
    assert got["mode"] == ("fork" if renderer.load_library().rt_device_count() >= 2 else "contexts")
    _assert_matches_one_context_and_oracle(W, oracle_lib, got)


@needs_node
@pytest.mark.gpu
def test_forked_rank_with_rccl_from_javascript_one_rank(W, oracle_lib, addon):
    """The forked mode with ONE rank (runs on one GPU): a fresh child, the unique id made in JavaScript, gatherStripes()."""
    from webgpu_raytracer_amd import renderer
    try:
        renderer.dist_unique_id()
    except W.RendererError as e:
        pytest.skip("RCCL could not be initialised here: %s" % e)
    env = dict(os.environ, RT_NODE_SHARDED_MODE="fork")
    got = run_json([os.path.join(NODE_DIR, "render_sharded.js"), "cornell", "96", "80", "7", "4", "1"], env=env, timeout=400)
    assert got["mode"] == "fork" and got["world"] == 1
    _assert_matches_one_context_and_oracle(W, oracle_lib, got)


@needs_node
@pytest.mark.gpu
def test_forked_rccl_ranks_on_two_gpus_from_javascript(W, oracle_lib, addon):
    from webgpu_raytracer_amd import renderer
    if renderer.load_library().rt_device_count() < 2:
        pytest.skip("needs two GPUs (RCCL refuses two ranks on one device)")
    env = dict(os.environ, RT_NODE_SHARDED_MODE="fork")
    got = run_json([os.path.join(NODE_DIR, "render_sharded.js"), "cornell", "96", "80", "7", "4", "2"], env=env, timeout=400)
    assert got["mode"] == "fork"
    _assert_matches_one_context_and_oracle(W, oracle_lib, got)
