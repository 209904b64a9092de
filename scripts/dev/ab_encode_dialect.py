#!/usr/bin/env python3
"""A/B of encode_batch(dialect="zig") against dialect="cxx" on the headline shape.

One device, one process: units x unit-bytes of synthetic data at each zero density, dense
outputs (sizes-only call, lengths_to_offsets, write). The two dialects are timed alternately
with device events, --reps repetitions after --warmup, and reported as medians; the Zig time
of the same run is the yardstick. Prints one JSON line per density.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "capnp-zig_amd"))

import torch  # noqa: E402

import capnp_packed as cp  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=1 << 20)
    ap.add_argument("--unit-bytes", type=int, default=4096)
    ap.add_argument("--densities", type=float, nargs="+", default=[0.5, 0.1, 0.9])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xC0DE0001)
    ap.add_argument("--out", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    n, ub = a.units, a.unit_bytes
    in_off, in_len = cp.uniform_layout(n, ub, device=dev)
    for p in a.densities:
        thr = round(p * 256)
        d_in = cp.generate(n, ub, seed=a.seed, zero_thresh=thr, device=dev)
        state = {}
        for d in ("zig", "cxx"):
            sz = torch.zeros(n, dtype=torch.int64, device=dev)
            st = torch.full((n,), -1, dtype=torch.int32, device=dev)
            cp.encoded_size_batch(d_in, in_off, in_len, sz, st, dialect=d)
            off = cp.lengths_to_offsets(sz)
            total = int(off[-1].item())
            assert int((st != 0).sum().item()) == 0
            state[d] = dict(cap=sz, off=off[:n].contiguous(), total=total,
                            out=torch.empty(total + 16, dtype=torch.uint8, device=dev),
                            ln=torch.zeros(n, dtype=torch.int64, device=dev), st=st, ms=[])

        def run(d):
            s = state[d]
            cp.encode_batch(d_in, in_off, in_len, s["out"], s["off"], s["cap"], s["ln"], s["st"], dialect=d)

        for _ in range(a.warmup):
            run("zig")
            run("cxx")
        torch.cuda.synchronize()
        for _ in range(a.reps):
            for d in ("zig", "cxx"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(d)
                e1.record()
                e1.synchronize()
                state[d]["ms"].append(e0.elapsed_time(e1))
        for d in ("zig", "cxx"):
            s = state[d]
            assert int((s["st"] != 0).sum().item()) == 0 and int(s["ln"].sum().item()) == s["total"]
        mz, mc = statistics.median(state["zig"]["ms"]), statistics.median(state["cxx"]["ms"])
        line = json.dumps({
            "units": n, "unit_bytes": ub, "p": p, "zero_thresh": thr, "reps": a.reps,
            "zig_ms_median": round(mz, 4), "cxx_ms_median": round(mc, 4), "ratio_cxx_over_zig": round(mc / mz, 4),
            "zig_ms_min_max": [round(min(state["zig"]["ms"]), 4), round(max(state["zig"]["ms"]), 4)],
            "cxx_ms_min_max": [round(min(state["cxx"]["ms"]), 4), round(max(state["cxx"]["ms"]), 4)],
            "zig_packed_bytes": state["zig"]["total"], "cxx_packed_bytes": state["cxx"]["total"],
            "unpacked_bytes": n * ub,
        })
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")
        del state, d_in
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
