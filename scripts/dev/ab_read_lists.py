"""list_heads_batch -> lengths_to_offsets -> read_elements_batch next to read_fields_batch
(DESIGN.md §2.14): device events, medians of 20 after warm-up, the legs alternating in one process.

Shape: --n (default 1048576) single-segment framed messages of 288 bytes. Each root (no data, one
pointer) holds a struct list of 8 elements of 2 data words and 1 pointer, a Text of 7 bytes and a
NUL. Fields per element: U64@0, U32@8, TEXT p0.
  legs: list_heads_batch, lengths_to_offsets, read_elements_batch (8 n elements)
  yardstick: read_fields_batch reading the same three kinds from 8 n messages of 48 bytes whose
             ROOT is such a struct (2 data words, 1 pointer, the same Text): the per-struct cost
             of the root read against the per-struct cost of the element read
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
ELEMS = 8
LIST_WORDS = 36   # header, root pointer, list pointer, tag, 8 x (2 data + 1 pointer), 8 texts
ROOT_WORDS = 6    # header, root pointer, 2 data, 1 pointer, the text


def struct_ptr(offset, data_words, pointers):
    return (offset << 2) | (data_words << 32) | (pointers << 48)


def list_ptr(offset, size, count):
    return 1 | (offset << 2) | (size << 32) | (count << 35)


TEXT = int.from_bytes(b"element\0", "little")


def tiled(template, n):
    rows = torch.from_numpy(np.asarray(template, dtype=np.uint64).view(np.int64)).to(DEV).repeat(n, 1)
    return rows


def list_batch(n):
    w = [0] * LIST_WORDS
    w[0] = (LIST_WORDS - 1) << 32
    w[1] = struct_ptr(0, 0, 1)
    w[2] = list_ptr(0, 7, 3 * ELEMS)
    w[3] = struct_ptr(ELEMS, 2, 1)
    for k in range(ELEMS):
        e = 4 + 3 * k
        w[e + 1] = 5 | (k << 32)
        w[e + 2] = list_ptr((28 + k) - (e + 2) - 1, 2, 8)
        w[28 + k] = TEXT
    rows = tiled(w, n)
    ids = torch.arange(n, dtype=torch.int64, device=DEV)
    for k in range(ELEMS):
        rows[:, 4 + 3 * k] = ids * ELEMS + k  # U64@0 of element k of message i
    off, ln = cp.uniform_layout(n, 8 * LIST_WORDS, device=DEV)
    return rows.view(-1).view(torch.uint8), off, ln


def root_batch(n):
    w = [(ROOT_WORDS - 1) << 32, struct_ptr(0, 2, 1), 0, 5, list_ptr(0, 2, 8), TEXT]
    rows = tiled(w, n)
    rows[:, 2] = torch.arange(n, dtype=torch.int64, device=DEV)
    off, ln = cp.uniform_layout(n, 8 * ROOT_WORDS, device=DEV)
    return rows.view(-1).view(torch.uint8), off, ln


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
    total = ELEMS * n
    fields = [cp.Field(cp.FIELD_U64, 0), cp.Field(cp.FIELD_U32, 8), cp.Field(cp.FIELD_TEXT, 0)]
    nf = len(fields)
    d, off, ln = list_batch(n)
    head = torch.zeros(n * cp.LIST_HEAD_BYTES, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(n, dtype=torch.int64, device=DEV)
    hst = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    start = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    out = torch.zeros(3, nf * total, dtype=torch.int64, device=DEV)
    st = torch.full((nf * total,), -1, dtype=torch.int32, device=DEV)
    num = torch.zeros(2, total, dtype=torch.int32, device=DEV)
    rd, roff, rln = root_batch(total)
    rout = torch.zeros(3, nf * total, dtype=torch.int64, device=DEV)
    rst = torch.full((nf * total,), -1, dtype=torch.int32, device=DEV)
    cp.list_heads_batch(d, off, ln, cp.LIST_STRUCT, 0, head, counts, hst)
    cp.lengths_to_offsets(counts, out=start)

    def elements(with_numbering=True):
        cp.read_elements_batch(d, off, ln, head, start, cp.LIST_STRUCT, total, fields, out[0], out[1], st, out[2],
                               num[0] if with_numbering else None, num[1] if with_numbering else None)

    res = {"n": n, "elements": total, "fields": nf, "list_message_bytes": 8 * LIST_WORDS,
           "root_message_bytes": 8 * ROOT_WORDS}
    res.update(alternate({
        "list_heads_ms": lambda: cp.list_heads_batch(d, off, ln, cp.LIST_STRUCT, 0, head, counts, hst),
        "lengths_to_offsets_ms": lambda: cp.lengths_to_offsets(counts, out=start),
        "read_elements_ms": elements,
        "read_elements_no_numbering_ms": lambda: elements(False),
        "read_fields_roots_ms": lambda: cp.read_fields_batch(rd, roff, rln, fields, rout[0], rout[1], rst, rout[2]),
    }))
    elements()
    torch.cuda.synchronize()
    assert (hst == cp.OK).all() and (counts == ELEMS).all() and int(start[n].item()) == total
    assert (st == cp.OK).all() and (rst == cp.OK).all()
    assert torch.equal(out[0][:total], torch.arange(total, dtype=torch.int64, device=DEV))
    assert torch.equal(num[0].long(), torch.arange(total, device=DEV) // ELEMS)
    assert torch.equal(num[1].long(), torch.arange(total, device=DEV) % ELEMS)
    assert (out[0][total:2 * total] == 5).all() and (out[1][2 * total:] == 7).all()
    assert torch.equal(rout[0][:total], torch.arange(total, dtype=torch.int64, device=DEV))
    assert (rout[1][2 * total:] == 7).all()
    res["chain_ms"] = res["list_heads_ms"] + res["lengths_to_offsets_ms"] + res["read_elements_ms"]
    res["ns_per_struct_elements"] = res["read_elements_ms"] * 1e6 / total
    res["ns_per_struct_chain"] = res["chain_ms"] * 1e6 / total
    res["ns_per_struct_roots"] = res["read_fields_roots_ms"] * 1e6 / total
    res["elements_over_roots"] = res["read_elements_ms"] / res["read_fields_roots_ms"]
    res["chain_over_roots"] = res["chain_ms"] / res["read_fields_roots_ms"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
