"""read_fields_batch and gather_batch next to their yardsticks: device events,
medians of 20 after warm-up, the two legs of each pair alternating in one process.

Shape: --n (default 1048576) single-segment framed messages of 4 KiB. Each root has 4 data words
and 2 pointers: a 16-byte Text and a Data field filling the rest of the message (4016 bytes).
Fields: U64@0, U32@8, U16@16, BOOL@24.3, TEXT p0, DATA p1.
  pair 1: read_fields_batch  vs  validate_batch on the same batch (a call of the parent commit
          that visits a superset of the words)
          plus, in the same alternation, the call with d_count NULL, with the four data fields
          only and with one data field: what the output columns cost (28 bytes per field and
          message against validate's 12 per message)
  pair 2: gather_batch of the DATA column into dense bytes  vs  a device-to-device copy_ of the
          same byte count (the yardstick of bench.py's copy_ceiling)
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "capnp-zig_amd"))
import capnp_packed as cp  # noqa: E402

DEV = "cuda"
FRAMED = 4096
WORDS = FRAMED // 8
TEXT_WORDS = 2
DATA_BYTES = 8 * (WORDS - 1 - 1 - 4 - 2 - TEXT_WORDS)  # header word, root pointer, data section, 2 pointers, text


def struct_ptr(offset, data_words, pointers):
    return (offset << 2) | (data_words << 32) | (pointers << 48)


def list_ptr(offset, size, count):
    return 1 | (offset << 2) | (size << 32) | (count << 35)


def batch(n):
    d = cp.generate(n, FRAMED, seed=0xF1E1D5, zero_thresh=128, device=DEV)
    head = np.zeros(9, dtype=np.uint64)
    head[0] = (WORDS - 1) << 32                      # one segment of 511 words
    head[1] = struct_ptr(0, 4, 2)                    # the root pointer
    head[6] = list_ptr(1, 2, 8 * TEXT_WORDS)         # p0: Text, right behind the pointer section
    head[7] = list_ptr(TEXT_WORDS, 2, DATA_BYTES)    # p1: Data, behind the text
    rows = d.view(torch.int64).view(n, WORDS)
    tmpl = torch.from_numpy(head.view(np.int64)).to(DEV)
    for k in (0, 1, 6, 7):  # words 2-5 (the data section) and the text / data bytes stay generated
        rows[:, k] = tmpl[k]
    off, ln = cp.uniform_layout(n, FRAMED, device=DEV)
    return d, off, ln


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
    d, off, ln = batch(n)
    fields = [cp.Field(cp.FIELD_U64, 0), cp.Field(cp.FIELD_U32, 8), cp.Field(cp.FIELD_U16, 16),
              cp.Field(cp.FIELD_BOOL, 24, 3), cp.Field(cp.FIELD_TEXT, 0), cp.Field(cp.FIELD_DATA, 1)]
    nf = len(fields)
    out = torch.zeros(3, nf * n, dtype=torch.int64, device=DEV)
    st = torch.full((nf * n,), -1, dtype=torch.int32, device=DEV)
    vst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    words = torch.zeros(n, dtype=torch.int64, device=DEV)
    res = {"n": n, "framed": FRAMED, "fields": nf}
    res.update(alternate({
        "read_fields_ms": lambda: cp.read_fields_batch(d, off, ln, fields, out[0], out[1], st, out[2]),
        "validate_ms": lambda: cp.validate_batch(d, off, ln, vst, words),
        "read_fields_no_count_ms": lambda: cp.read_fields_batch(d, off, ln, fields, out[0], out[1], st),
        "read_fields_4_data_fields_ms": lambda: cp.read_fields_batch(d, off, ln, fields[:4], out[0], out[1], st,
                                                                     out[2]),
        "read_fields_1_data_field_ms": lambda: cp.read_fields_batch(d, off, ln, fields[:1], out[0], out[1], st,
                                                                    out[2]),
    }))
    cp.read_fields_batch(d, off, ln, fields, out[0], out[1], st, out[2])  # all six again for the checks below
    assert (st == cp.OK).all() and (vst == cp.OK).all()
    data_len = out[1][5 * n:6 * n]
    assert (data_len == DATA_BYTES).all() and (out[1][4 * n:5 * n] <= 8 * TEXT_WORDS).all()
    res["read_fields_over_validate"] = res["read_fields_ms"] / res["validate_ms"]
    res["read_fields_output_mb"] = nf * n * 28 / 1e6
    res["validate_output_mb"] = n * 12 / 1e6

    total = DATA_BYTES * n
    src_off = out[0][5 * n:6 * n]
    dst_off = cp.lengths_to_offsets(data_len)
    dense = torch.empty(total, dtype=torch.uint8, device=DEV)
    flat = torch.empty(total, dtype=torch.uint8, device=DEV)
    gst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    res.update(alternate({
        "gather_ms": lambda: cp.gather_batch(d, src_off, data_len, dense, dst_off, gst, cap=total),
        "copy_ms": lambda: flat.copy_(d[:total]),
    }))
    assert (gst == cp.OK).all()
    k = n // 3  # one message's bytes arrived
    lo = int(src_off[k].item())
    assert torch.equal(dense[k * DATA_BYTES:(k + 1) * DATA_BYTES], d[lo:lo + DATA_BYTES])
    res["gather_bytes"] = total
    res["gather_gib_s"] = 2 * total / res["gather_ms"] / 1e-3 / 2**30
    res["copy_gib_s"] = 2 * total / res["copy_ms"] / 1e-3 / 2**30
    res["gather_over_copy_bandwidth"] = res["copy_ms"] / res["gather_ms"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
