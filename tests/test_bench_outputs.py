"""`bench.py --dump-outputs DIR`: the outputs of the last timed image, written after the timed steps, are what the
renderer computes for the headline workload (bit for bit), and `--steps` is the number of timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
QUICK = ["--no-extra-configs", "--no-cpu-baseline", "--no-live-loop", "--no-world-update"]


def test_bench_refuses_zero_steps():
    out = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--steps must be at least 1" in out.stderr


def test_dump_writes_the_accumulation_and_a_fixed_frame_sample(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    accum = rng.random((bench.HEIGHT, bench.WIDTH, 4), dtype=np.float32)
    frame = rng.integers(0, 256, (bench.HEIGHT, bench.WIDTH, 4), dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), accum, frame)
    bench.dump_outputs(str(tmp_path / "b"), accum, frame)
    for d in ("a", "b"):
        assert sorted(os.listdir(tmp_path / d)) == ["accum.npy", "frame_sample.npy"]
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 64 * 10**6
    a = np.load(tmp_path / "a" / "accum.npy")
    assert a.dtype == np.float32 and np.array_equal(a, accum)
    s = np.load(tmp_path / "a" / "frame_sample.npy")
    assert s.dtype == np.float32 and s.shape == (bench.HEIGHT * bench.WIDTH // 4, 4)
    assert np.array_equal(s, np.load(tmp_path / "b" / "frame_sample.npy"))      # the same pixels every run
    assert set(map(tuple, s.astype(np.uint8))) <= set(map(tuple, frame.reshape(-1, 4)))


@pytest.mark.gpu
def test_dumped_outputs_are_the_headline_image(W, tmp_path):
    import bench
    W._build.build_rt()
    dump = tmp_path / "out"
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(dump)]
                         + QUICK, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][0])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0
    files = sorted(os.listdir(dump))
    assert files == ["accum.npy", "frame_sample.npy"]
    got = {f[:-4]: np.load(dump / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6

    # the same images in this process: bench.py's headline step, once per warmup and timed step (present() blends with
    # the history of the frames presented before it, so the last frame depends on all of them; the accumulation does not)
    b = W.WorldBridge()
    b.loadScene(bench.SCENE)
    r = W.WebGPURenderer(0)
    r.buildPipeline(bench.DEPTH, 1)
    W.upload_scene(r, b, bench.WIDTH, bench.HEIGHT)
    frames = list(range(1, bench.SPP_TOTAL + 1))
    for _ in range(1 + 2):
        r.resetAccumulation()
        for i in range(0, len(frames), 32):
            r.computeBatch(frames[i:i + 32])
        r.present()
    r.sync()
    accum, frame = r.readAccum(), r.captureFrame()["data"].copy()
    r.destroy()
    assert got["accum"].shape == (bench.HEIGHT, bench.WIDTH, 4)
    assert np.array_equal(got["accum"].view(np.uint32), accum.view(np.uint32))
    px = bench.WIDTH * bench.HEIGHT
    pick = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(px, px // 4, replace=False))
    assert np.array_equal(got["frame_sample"], frame.reshape(px, 4)[pick].astype(np.float32))


@pytest.mark.gpu
def test_a_plain_run_prints_the_headline_alone(W):
    """Without --full the benchmark times the headline and prints its line; the roofline, the other configs, the live
    loop, the world update and the CPU baseline come with --full only."""
    W._build.build_rt()
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "1", "--warmup", "0"],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["unit"] == "Mrays/s" and rec["value"] > 0 and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == 1 and rec["warmup"] == 0 and rec["ms_per_step"] > 0
    assert not {"roofline", "configs", "live_loop", "live_loop_animated", "world_update", "cpu_baseline"} & set(rec)
