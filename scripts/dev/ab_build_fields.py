"""build_fields_batch next to its yardsticks: device events, medians of 20
after warm-up, the legs alternating in one process.

Shape: §2.13's. --n (default 1048576) messages of 4 KiB framed: a root of 4 data words and 2
pointers, a 16-byte Text and a 4016-byte Data. Ops: STRUCT(4, 2), U64@0, U32@8, U16@16,
BOOL@24.3, TEXT p0, DATA p1. The slices come from a pool in which message i's Text and Data lie
back to back.
  leg 1: build_fields_batch
  leg 2: gather_batch of the same DATA column into the same destination layout (each Data at
         the place it has inside its message)
  leg 3: a device copy_ of as many bytes as the build writes
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "capnp-zig_amd"))
import capnp_packed as cp  # noqa: E402

DEV = "cuda"
FRAMED = 4096
TEXT_BYTES = 15           # + NUL: 16 bytes, two words
DATA_BYTES = 4016
DATA_AT = 8 * (1 + 1 + 4 + 2 + 2)  # table, root pointer, data section, pointers, text
ROW = TEXT_BYTES + DATA_BYTES      # pool bytes per message


def alternate(legs, reps=20, warm=3):
    """median ms of each leg, the legs taking turns"""
    for _ in range(warm):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: statistics.median(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    a = ap.parse_args()
    n = a.n
    assert DATA_AT + DATA_BYTES == FRAMED
    pool = cp.generate(n, ROW + 1, seed=0xB111D, zero_thresh=0, device=DEV)[:n * ROW + 64]
    ops = [cp.BuildOp(cp.BUILD_STRUCT, 0, data_words=4, pointer_words=2), cp.BuildOp(cp.FIELD_U64, 0),
           cp.BuildOp(cp.FIELD_U32, 8), cp.BuildOp(cp.FIELD_U16, 16), cp.BuildOp(cp.FIELD_BOOL, 24, 3),
           cp.BuildOp(cp.FIELD_TEXT, 0), cp.BuildOp(cp.FIELD_DATA, 1)]
    nops = len(ops)
    idx = torch.arange(n, dtype=torch.int64, device=DEV)
    value = torch.zeros(nops, n, dtype=torch.int64, device=DEV)
    length = torch.zeros(nops, n, dtype=torch.int64, device=DEV)
    for k in range(1, 5):
        value[k] = idx * (2 * k + 1) + k
    value[5], length[5] = idx * ROW, TEXT_BYTES
    value[6], length[6] = idx * ROW + TEXT_BYTES, DATA_BYTES
    out_off, out_cap = cp.uniform_layout(n, FRAMED, device=DEV)
    out_len = torch.zeros(n, dtype=torch.int64, device=DEV)
    st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    built = torch.empty(n * FRAMED, dtype=torch.uint8, device=DEV)
    gathered = torch.empty(n * FRAMED, dtype=torch.uint8, device=DEV)
    flat = torch.empty(n * FRAMED, dtype=torch.uint8, device=DEV)
    src = torch.empty(n * FRAMED, dtype=torch.uint8, device=DEV)
    gst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    data_dst = out_off + DATA_AT
    v, l = value.view(-1), length.view(-1)
    res = {"n": n, "framed": FRAMED, "ops": nops}
    res.update(alternate({
        "build_ms": lambda: cp.build_fields_batch(pool, ops, v, l, built, out_off, out_cap, out_len, st,
                                                  pool_len=n * ROW),
        "gather_ms": lambda: cp.gather_batch(pool, value[6], length[6], gathered, data_dst, gst),
        "copy_ms": lambda: flat.copy_(src),
    }))
    assert (st == cp.OK).all() and (gst == cp.OK).all() and (out_len == FRAMED).all()
    k = n // 3  # one message: the gather's bytes are the build's Data, and the message validates
    assert torch.equal(built[k * FRAMED + DATA_AT:(k + 1) * FRAMED], gathered[k * FRAMED + DATA_AT:(k + 1) * FRAMED])
    vst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.validate_batch(built, out_off, out_len, vst)
    assert (vst == cp.OK).all()
    res["build_over_gather"] = res["build_ms"] / res["gather_ms"]
    res["build_over_copy"] = res["build_ms"] / res["copy_ms"]
    res["build_bytes_written"] = n * FRAMED
    res["gather_bytes_written"] = n * DATA_BYTES
    res["build_gib_s"] = (n * FRAMED + n * ROW) / res["build_ms"] / 1e-3 / 2**30
    res["copy_gib_s"] = 2 * n * FRAMED / res["copy_ms"] / 1e-3 / 2**30
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
