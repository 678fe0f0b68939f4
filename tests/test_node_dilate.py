"""Atlas dilation driven from JavaScript (WebGPURenderer.dilateAtlas of node/index.js): one 65 x 63 atlas through the addon
equals the reference model word for word - atlas, source map and count - and the input array is left as it was."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import dilate_util as du

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")

SCRIPT = """
const fs = require('fs');
const { WebGPURenderer } = require(process.argv[1] + '/index.js');
const [inPath, outPath, srcPath, width, height, radius] = process.argv.slice(2);
(async () => {
  const buf = fs.readFileSync(inPath);
  const atlas = new Float32Array(buf.buffer, buf.byteOffset, buf.length / 4);
  const before = Uint32Array.from(new Uint32Array(buf.buffer, buf.byteOffset, buf.length / 4));
  const r = new WebGPURenderer(0);
  await r.init();
  const res = r.dilateAtlas(atlas, +width, +height, +radius, { src: true });
  r.destroy();
  const after = new Uint32Array(buf.buffer, buf.byteOffset, buf.length / 4);
  fs.writeFileSync(outPath, Buffer.from(res.data.buffer));
  fs.writeFileSync(srcPath, Buffer.from(res.src.buffer));
  console.log(JSON.stringify({ filled: res.filled, width: res.width, height: res.height,
    inputKept: before.every((w, i) => w === after[i]) }));
})().catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_dilation_matches_the_model(W, tmp_path):
    W._build.build_rt()
    assert W._build.build_node_addon()
    width, height, p, seed, radius = 65, 63, 0.05, 1, 7
    atlas = du.pattern(width, height, p, seed)
    want, want_src, filled, _ = du.dilate_model(atlas, radius)
    assert filled == du.PATTERNS[(width, height, p, seed, radius)][1]
    in_path, out_path, src_path = tmp_path / "atlas.f32", tmp_path / "out.f32", tmp_path / "src.u32"
    atlas.tofile(str(in_path))
    out = subprocess.run([node, "-e", SCRIPT, NODE_DIR, str(in_path), str(out_path), str(src_path), str(width), str(height),
                          str(radius)], check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    assert info == {"filled": filled, "width": width, "height": height, "inputKept": True}
    got = np.fromfile(str(out_path), dtype=np.uint32).reshape(height, width, 4)
    assert np.array_equal(got, du.words(want))
    assert np.array_equal(np.fromfile(str(src_path), dtype=np.uint32).reshape(height, width), want_src)
