#!/usr/bin/env python3
"""A/B of the ways to a dense packed stream.

One device, one process, the paths timed alternately with device events, --reps repetitions
after --warmup, medians reported:
  (a) three calls: encoded_size_batch -> lengths_to_offsets -> encode_batch(dense offsets);
  (b) encode_batch into capacity slots of encode_bound(len) (not a dense stream: the yardstick);
  (c) encode_dense_batch, dialect "zig" and "cxx".
Shapes: units x unit-bytes at each zero density, and config C5's skewed sizes (--c5; p = 0.5).
(c)'s stream is compared with (a)'s once per shape. Prints one JSON line per shape.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "capnp-zig_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import capnp_packed as cp  # noqa: E402


def pareto_sizes(n, seed=0xC0DE0005):
    """Config C5 (bench.py): a truncated Pareto, 64 B .. 256 KiB, mean ~424 B."""
    u = np.random.default_rng(seed).random(n)
    return (8 * np.floor(np.clip(64.0 * (1.0 - u) ** (-1.0 / 1.1), 64, 262144) / 8)).astype(np.int64)


def measure(name, d_in, in_off, in_len, a, dev, extra):
    n = in_off.numel()
    i64 = dict(dtype=torch.int64, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    # (a) three calls
    a_len, a_ln2 = torch.zeros(n, **i64), torch.zeros(n, **i64)
    scratch = torch.empty(cp.lib().capnp_packed_scan_scratch_bytes(n) // 8 + 1, **i64)
    a_off = torch.zeros(n + 1, **i64)
    cp.encoded_size_batch(d_in, in_off, in_len, a_len, st)
    total = int(cp.lengths_to_offsets(a_len)[-1].item())
    a_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)

    def run_a():
        cp.encoded_size_batch(d_in, in_off, in_len, a_len, st)
        cp._raise(cp.lib().capnp_packed_lengths_to_offsets(a_len.data_ptr(), n, 0, a_off.data_ptr(),
                                                            scratch.data_ptr(), scratch.numel() * 8,
                                                            torch.cuda.current_stream().cuda_stream), "scan")
        cp.encode_batch(d_in, in_off, in_len, a_out, a_off, a_len, a_ln2, st)

    # (b) capacity slots
    caps = (in_len // 8) * 10
    slots = (caps + 15) // 16 * 16
    b_off = torch.zeros(n, **i64)
    b_off[1:] = torch.cumsum(slots, 0)[:-1]
    b_out = torch.empty(int(slots.sum().item()), dtype=torch.uint8, device=dev)
    b_len = torch.zeros(n, **i64)

    def run_b():
        cp.encode_batch(d_in, in_off, in_len, b_out, b_off, caps, b_len, st)

    # (c) the dense call
    ws = cp.dense_workspace(n, device=dev)
    c_out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    c_off, c_len = torch.zeros(n + 1, **i64), torch.zeros(n, **i64)
    c_st = torch.full((n,), -1, dtype=torch.int32, device=dev)

    def run_c(dialect):
        cp.encode_dense_batch(d_in, in_off, in_len, c_out, c_off, c_len, c_st, ws=ws, dialect=dialect)

    paths = {"three_call": run_a, "slots": run_b, "dense_zig": lambda: run_c("zig"),
             "dense_cxx": lambda: run_c("cxx")}
    # one check per shape: (c) writes (a)'s stream
    run_a()
    run_c("zig")
    torch.cuda.synchronize()
    for what, s in (("three-call", st), ("dense", c_st)):
        bad = torch.nonzero(s != 0).flatten()
        assert bad.numel() == 0, (f"{what}: {bad.numel()} units not OK, first {bad[:8].tolist()} with status "
                                  f"{s[bad[:8]].tolist()}; workspace head {ws[:4].tolist()}")
    if not a.no_check:
        assert torch.equal(c_off, a_off) and torch.equal(c_out[:total], a_out[:total]), "dense stream differs"
    wait_us = int(ws[2].item()) / 100.0
    run_c("cxx")
    torch.cuda.synchronize()
    cxx_total = int(c_off[-1].item())
    assert int((c_st != 0).sum().item()) == 0

    ms = {k: [] for k in paths}
    for _ in range(a.warmup):
        for f in paths.values():
            f()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {"shape": name, "units": n, "unpacked_bytes": int(in_len.sum().item()), "reps": a.reps, **extra}
    for k in paths:
        line[k + "_ms_median"] = round(med[k], 4)
        line[k + "_ms_min_max"] = [round(min(ms[k]), 4), round(max(ms[k]), 4)]
    line["dense_over_three_call"] = round(med["dense_zig"] / med["three_call"], 4)
    line["dense_over_slots"] = round(med["dense_zig"] / med["slots"], 4)
    line["dense_cxx_over_three_call"] = round(med["dense_cxx"] / med["three_call"], 4)
    line["packed_bytes"] = total
    line["packed_bytes_cxx"] = cxx_total
    line["slot_bytes"] = int(b_out.numel())
    line["longest_lookback_wait_us"] = wait_us
    return line


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=1 << 20)
    ap.add_argument("--unit-bytes", type=int, default=4096)
    ap.add_argument("--densities", type=float, nargs="*", default=[0.5, 0.1, 0.9])
    ap.add_argument("--c5", action="store_true", help="also config C5's skewed sizes (p = 0.5)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xC0DE0001)
    ap.add_argument("--no-check", action="store_true", help="diagnostic builds: skip the stream comparison")
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    lines = []
    n, ub = a.units, a.unit_bytes
    for p in a.densities:
        thr = round(p * 256)
        in_off, in_len = cp.uniform_layout(n, ub, device=dev)
        d_in = cp.generate(n, ub, seed=a.seed, zero_thresh=thr, device=dev)
        lines.append(measure("uniform", d_in, in_off, in_len, a, dev, {"unit_bytes": ub, "p": p}))
        print(json.dumps(lines[-1]), flush=True)
        del d_in
        torch.cuda.empty_cache()
    if a.c5:
        sizes = torch.from_numpy(pareto_sizes(n)).to(dev)
        in_off = torch.zeros(n, dtype=torch.int64, device=dev)
        in_off[1:] = torch.cumsum(sizes, 0)[:-1]
        d_in = cp.generate(1, int(sizes.sum().item()), seed=0xC0DE0005, zero_thresh=128, device=dev)
        lines.append(measure("c5_skewed", d_in, in_off, sizes, a, dev, {"p": 0.5}))
        print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
