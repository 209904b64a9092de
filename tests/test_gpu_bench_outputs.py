"""A plain `bench.py --gpus 1` run and its `--dump-outputs DIR`: the result line carries the
headline fields and none of the `--full` measurements, `--steps` is the number of timed steps,
and the dumped arrays (float32 / float64 .npy files of what encode_batch / decode_batch left in
the caller's buffers at the last timed step) equal the oracle's results for the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, UB, SEED, THR = 768, 4096, 0xC0DE001B, 128
FULL_ONLY = ("sweep", "dense_stream", "read_message", "message_framing", "rpc_framer", "rpc_framer_split",
             "c5_skewed", "validate", "c1_bench_message", "host_path", "cpu_baseline")


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out_dir = str(tmp_path_factory.mktemp("dump"))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--units", str(N), "--unit-bytes", str(UB), "--seed", str(SEED), "--zero-thresh", str(THR),
                          "--dump-outputs", out_dir], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in os.listdir(out_dir) if f.endswith(".npy")}
    nbytes = sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir))
    return json.loads(lines[0]), arrays, nbytes


def test_plain_run_reports_the_headline_only(plain_run):
    res, _, _ = plain_run
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["bit_exact_roundtrip"]
    assert res["unit"] == "GiB/s" and res["higher_is_better"] is True and res["dtype"] == "u8"
    assert res["ms_per_step"] > 0
    # value is the unpacked bytes of one step over ms_per_step
    assert res["value"] == pytest.approx(N * UB / (res["ms_per_step"] * 1e-3) / 2 ** 30, rel=1e-2)
    assert not [k for k in FULL_ONLY if k in res] and res["roofline"]["ceilings_GBps"] is None


def test_dumped_outputs_equal_the_oracle(plain_run):
    _, a, nbytes = plain_run
    assert nbytes <= 64_000_000
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    data = oracle.generate(N, UB, seed=SEED, zero_thresh=THR)
    packed = [oracle.pack(data[i * UB:(i + 1) * UB].tobytes())[1] for i in range(N)]
    assert np.array_equal(a["packed_len"], np.array([len(p) for p in packed], dtype=np.float64))
    assert np.array_equal(a["unpacked_len"], np.full(N, UB, dtype=np.float64))
    assert not a["encode_status"].any() and not a["decode_status"].any()
    assert a["encode_status"].shape == a["decode_status"].shape == (N,)
    assert a["packed_totals"].tolist() == [float(sum(len(p) for p in packed))]
    idx = a["sample_index"].astype(np.int64)
    slot = 10 * UB // 8
    assert len(idx) == len(set(idx.tolist())) > 0 and a["packed_bytes"].shape == (len(idx), slot)
    assert a["unpacked_bytes"].shape == (len(idx), UB)
    for row, i in enumerate(idx):
        want = np.zeros(slot, dtype=np.float32)
        want[:len(packed[i])] = np.frombuffer(packed[i], dtype=np.uint8)
        assert np.array_equal(a["packed_bytes"][row], want), f"unit {i}: packed bytes"
        assert np.array_equal(a["unpacked_bytes"][row], data[i * UB:(i + 1) * UB].astype(np.float32)), f"unit {i}"
