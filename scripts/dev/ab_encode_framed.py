#!/usr/bin/env python3
"""A/B of the framed-message encoders under the C++ dialect.

One device, one process, the paths timed alternately with device events, --reps repetitions
after --warmup, medians reported. Messages of 512 framed words at zero density --p:
  (a) single-segment messages (1 table word + 511): encode_framed_batch against encode_batch on
      the same bytes (the framed call should cost the table check and no more);
  (b) the same messages cut into 4 segments (3 table words + 128 + 127 + 127 + 127):
      encode_framed_batch and encode_framed_dense_batch against today's route
      message_init_batch -> device addresses -> encode_message_batch sizes -> lengths_to_offsets
      -> encode_message_batch (rows of 4 entries, the kindest the route can get: 512 would be
      16 KiB of tables a message).
Every path's bytes are compared once. Prints one JSON line per shape.
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

UB = 4096


def messages(n, table, seed, p, dev):
    """n units of 4096 random bytes whose first words are the segment table `table` (u32s)."""
    d_in = cp.generate(n, UB, seed=seed, zero_thresh=round(p * 256), device=dev)
    rows = d_in.view(torch.int32).view(n, UB // 4)
    rows[:, :len(table)] = torch.tensor(table, dtype=torch.int32, device=dev)
    return d_in


def timed(paths, a):
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
    out = {}
    for k, v in ms.items():
        out[k + "_ms_median"] = round(statistics.median(v), 4)
        out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--units", type=int, default=1 << 20)
    ap.add_argument("--p", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xC0DE0001)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("no GPU: nothing measured", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    n = a.units
    i64 = dict(dtype=torch.int64, device=dev)
    in_off, in_len = cp.uniform_layout(n, UB, device=dev)
    slot = cp.encode_bound(UB)
    s_off, s_cap = cp.uniform_layout(n, slot, device=dev)
    out_a = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    out_b = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    len_a, len_b = torch.zeros(n, **i64), torch.zeros(n, **i64)
    st_a = torch.full((n,), -1, dtype=torch.int32, device=dev)
    st_b = torch.full((n,), -1, dtype=torch.int32, device=dev)
    fws = cp.framed_workspace(n, device=dev)

    # ---- (a) single-segment messages
    d_in = messages(n, [0, 511], a.seed, a.p, dev)
    paths = {
        "framed_batch": lambda: cp.encode_framed_batch(d_in, in_off, in_len, out_a, s_off, s_cap, len_a, st_a,
                                                       ws=fws, dialect="cxx"),
        "encode_batch": lambda: cp.encode_batch(d_in, in_off, in_len, out_b, s_off, s_cap, len_b, st_b,
                                                dialect="cxx"),
    }
    out_a.zero_()
    out_b.zero_()
    for f in paths.values():
        f()
    torch.cuda.synchronize()
    assert (st_a == 0).all().item() and (st_b == 0).all().item()
    assert torch.equal(len_a, len_b) and torch.equal(out_a, out_b), "single-segment bytes differ"
    line = {"shape": "single_segment", "units": n, "p": a.p, "reps": a.reps, **timed(paths, a)}
    line["framed_over_encode_batch"] = round(line["framed_batch_ms_median"] / line["encode_batch_ms_median"], 4)
    print(json.dumps(line), flush=True)

    # ---- (b) four segments
    d_in = messages(n, [3, 128, 127, 127, 127, 0], a.seed, a.p, dev)
    ms_rows = 4
    seg_count = torch.zeros(n, dtype=torch.int32, device=dev)
    seg_off, seg_len = torch.zeros(n * ms_rows, **i64), torch.zeros(n * ms_rows, **i64)
    seg_ptr = torch.zeros(n * ms_rows, **i64)
    seg_first = torch.arange(n, dtype=torch.int32, device=dev) * ms_rows
    st_i = torch.full((n,), -1, dtype=torch.int32, device=dev)
    sz = torch.zeros(n, **i64)
    d_off = torch.zeros(n + 1, **i64)
    scratch = torch.empty(cp.lib().capnp_packed_scan_scratch_bytes(n) // 8 + 1, **i64)
    base = d_in.data_ptr()

    def route(out, off, cap, ln, scan):
        cp.message_init_batch(d_in, in_off, in_len, ms_rows, seg_count, seg_off, seg_len, st_i)
        torch.add(seg_off.view(n, ms_rows), (in_off + base).view(n, 1), out=seg_ptr.view(n, ms_rows))
        if scan:  # a dense stream: sizes, the scan, then the bytes at exact offsets
            cp.encode_message_batch(seg_ptr, seg_len, seg_first, seg_count, None, None, None, sz, st_b, dialect="cxx")
            cp._raise(cp.lib().capnp_packed_lengths_to_offsets(sz.data_ptr(), n, 0, d_off.data_ptr(),
                                                                scratch.data_ptr(), scratch.numel() * 8,
                                                                torch.cuda.current_stream().cuda_stream), "scan")
            cp.encode_message_batch(seg_ptr, seg_len, seg_first, seg_count, out, d_off, sz, ln, st_b, dialect="cxx")
        else:
            cp.encode_message_batch(seg_ptr, seg_len, seg_first, seg_count, out, off, cap, ln, st_b, dialect="cxx")

    dws = cp.dense_workspace(n, device=dev)
    dn_out = torch.empty(n * slot, dtype=torch.uint8, device=dev)
    dn_off, dn_len = torch.zeros(n + 1, **i64), torch.zeros(n, **i64)
    dn_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    paths = {
        "framed_batch": lambda: cp.encode_framed_batch(d_in, in_off, in_len, out_a, s_off, s_cap, len_a, st_a,
                                                       ws=fws, dialect="cxx"),
        "route_slots": lambda: route(out_b, s_off, s_cap, len_b, False),
        "framed_dense": lambda: cp.encode_framed_dense_batch(d_in, in_off, in_len, dn_out, dn_off, dn_len, dn_st,
                                                             ws=dws, dialect="cxx"),
        "route_dense": lambda: route(out_b, None, None, len_b, True),
    }
    out_a.zero_()
    out_b.zero_()
    paths["framed_batch"]()
    paths["route_slots"]()
    torch.cuda.synchronize()
    assert (st_a == 0).all().item() and (st_b == 0).all().item() and (st_i == 0).all().item()
    assert torch.equal(len_a, len_b) and torch.equal(out_a, out_b), "four-segment bytes differ"
    paths["framed_dense"]()
    paths["route_dense"]()
    torch.cuda.synchronize()
    total = int(dn_off[n].item())
    assert (dn_st == 0).all().item() and torch.equal(dn_off, d_off) and torch.equal(dn_out[:total], out_b[:total])
    line = {"shape": "four_segments", "units": n, "p": a.p, "reps": a.reps, "packed_bytes": total, **timed(paths, a)}
    line["framed_over_route_slots"] = round(line["framed_batch_ms_median"] / line["route_slots_ms_median"], 4)
    line["framed_dense_over_route_dense"] = round(line["framed_dense_ms_median"] / line["route_dense_ms_median"], 4)
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
