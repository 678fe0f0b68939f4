"""node/gather_probes.js: probe gathers driven from JavaScript (WebGPURenderer.gatherProbes of node/index.js) equal the Python
binding's on the same probes, and the reference model."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_util as pu
import probe_util as prb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_probe_gathers_match_python(W, tmp_path):
    from webgpu_raytracer_amd import renderer as R
    W._build.build_rt()
    assert W._build.build_node_addon()
    b = pu.bridge_for(W, "cornell")
    m = prb.model_for(W, b)
    probes = prb.scene_probes(m, b)
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        want, st = r.gatherProbes(probes, 4, 65, prb.SEED, stats=True)
    finally:
        r.destroy()
    ref, _, counts = m.gatherProbes(probes, 4, 65, prb.SEED)
    prb.check_against_model(want, ref, "python")
    probes_path, out_path = tmp_path / "probes.bin", tmp_path / "out.f32"
    probes.tofile(str(probes_path))
    out = subprocess.run([node, os.path.join(NODE_DIR, "gather_probes.js"), "cornell", str(probes_path), str(out_path), "4",
                          "65", str(prb.SEED)], check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    got = np.fromfile(str(out_path), dtype=R.PROBE_SH9_DTYPE)
    assert got.shape[0] == probes.shape[0] == info["probes"]
    assert np.array_equal(prb.result_words(got), prb.result_words(want))
    for name in ("rays", "samples") + prb.COUNT_NAMES + ("lds",):
        assert info["stats"][name] == st[name], name
    prb.check_counts(info["stats"], counts, probes.shape[0], 65, "node")
