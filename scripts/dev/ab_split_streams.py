"""split_streams next to its references: device events, medians of 20 after
warm-up, one process.

Shapes (4 KiB framed messages, bytes zero with p = 0.5):
  1. S streams x 16 messages          (--streams, default 4096: the rpc_framer leg's shape)
  2. N streams x 1 message            (--wide, default 1048576)
  3. 1 stream x M messages            (--serial, default 65536)
References:
  (a) decoded_size_batch over the same bytes with the boundaries given (what a walk costs when
      nothing has to be found);
  (b) the whole-stream loop on the CPU through the oracle's reader, one thread, on --cpu-msgs
      messages (ctypes call per message included), scaled to the shape;
  (c) shape 1: read_message_batch called 16 times with the offsets advanced on the device
      (today's only device route; it also writes the frames).
Prints one JSON line per shape.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "capnp-zig_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import capnp_packed as cp  # noqa: E402
import oracle  # noqa: E402

DEV = "cuda"
FRAMED = 4096


def median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def dense_stream(n_msgs, seed):
    """n_msgs framed one-segment messages packed into one dense stream: (d_pk, off[n + 1], len[n])."""
    d = cp.generate(n_msgs, FRAMED, seed=seed, zero_thresh=128, device=DEV)
    head = np.zeros(8, dtype=np.uint8)
    head[4:8] = np.frombuffer(np.uint32(FRAMED // 8 - 1).tobytes(), dtype=np.uint8)
    d.view(n_msgs, FRAMED)[:, :8] = torch.from_numpy(head).to(DEV)
    in_off, in_len = cp.uniform_layout(n_msgs, FRAMED, device=DEV)
    d_pk = torch.empty(n_msgs * FRAMED * 3 // 4 + (1 << 20), dtype=torch.uint8, device=DEV)  # p = 0.5 packs to ~0.63
    off = torch.empty(n_msgs + 1, dtype=torch.int64, device=DEV)
    ln = torch.empty(n_msgs, dtype=torch.int64, device=DEV)
    st = torch.empty(n_msgs, dtype=torch.int32, device=DEV)
    cp.encode_dense_batch(d, in_off, in_len, d_pk, off, ln, st)
    torch.cuda.synchronize()
    assert (st == cp.OK).all()
    return d_pk, off, ln


def cpu_loop_us_per_msg(d_pk, off, n):
    """The oracle reader's whole-stream loop over the first n messages: microseconds a message."""
    end = int(off[n].item())
    held = d_pk[:end].cpu().numpy().tobytes()
    src = ctypes.create_string_buffer(held, len(held))
    dst = ctypes.create_string_buffer(FRAMED + 64)
    ln, used = ctypes.c_size_t(), ctypes.c_size_t()
    f = oracle.lib().oracle_read_packed_message
    base = ctypes.addressof(src)
    t0 = time.perf_counter()
    pos = k = 0
    while pos < end:
        rc = f(base + pos, end - pos, dst, FRAMED + 64, ctypes.byref(ln), ctypes.byref(used))
        assert rc == 0
        pos += used.value
        k += 1
    dt = time.perf_counter() - t0
    assert k == n
    return dt / n * 1e6


def shape(name, d_pk, off, ln, per_stream, cpu_us, with_rounds=False):
    n_msgs = ln.numel()
    n = n_msgs // per_stream
    s_off = off[:-1][::per_stream].contiguous()
    s_len = (off[per_stream::per_stream] - s_off).contiguous()
    total = int(off[n_msgs].item())
    first = torch.empty(n + 1, dtype=torch.int64, device=DEV)
    tab = torch.empty((3, n_msgs), dtype=torch.int64, device=DEV)
    consumed = torch.empty(n, dtype=torch.int64, device=DEV)
    status = torch.empty(n, dtype=torch.int32, device=DEV)
    res = {"shape": name, "streams": n, "msgs_per_stream": per_stream, "packed_bytes": total}
    for label, bound in (("split_ms", total), ("split_no_tables_ms", 0)):
        ws = cp.split_workspace(n, bound, device=DEV)
        res[label] = median_ms(lambda: cp.split_streams(d_pk, s_off, s_len, first, tab[0], tab[1], tab[2], consumed,
                                                        status, ws=ws))
        assert int(first[n].item()) == n_msgs and (status == cp.OK).all()
        assert torch.equal(tab[0], off[:-1]) and torch.equal(tab[1], ln)
    res["us_per_msg_per_stream"] = res["split_ms"] * 1e3 / per_stream
    sz = torch.empty(n_msgs, dtype=torch.int64, device=DEV)
    st = torch.empty(n_msgs, dtype=torch.int32, device=DEV)
    res["decoded_size_known_boundaries_ms"] = median_ms(
        lambda: cp.decoded_size_batch(d_pk, off[:-1], ln, sz, st))
    res["cpu_loop_1_thread_ms"] = cpu_us * n_msgs / 1e3
    if with_rounds:
        d_out = torch.empty(n * FRAMED, dtype=torch.uint8, device=DEV)
        o_off, o_cap = cp.uniform_layout(n, FRAMED, device=DEV)
        o_len = torch.empty(n, dtype=torch.int64, device=DEV)
        used = torch.empty(n, dtype=torch.int64, device=DEV)
        rst = torch.empty(n, dtype=torch.int32, device=DEV)

        def rounds():
            cur, left = s_off.clone(), s_len.clone()
            for _ in range(per_stream):
                cp.read_message_batch(d_pk, cur, left, d_out, o_off, o_cap, o_len, used, rst)
                cur += used
                left -= used

        res["read_message_batch_x%d_ms" % per_stream] = median_ms(rounds, reps=10)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--wide", type=int, default=1 << 20)
    ap.add_argument("--serial", type=int, default=1 << 16)
    ap.add_argument("--cpu-msgs", type=int, default=4096)
    a = ap.parse_args()
    d_pk, off, ln = dense_stream(max(a.streams, 1) * 16, 0x5B110001)
    cpu_us = cpu_loop_us_per_msg(d_pk, off, min(a.cpu_msgs, ln.numel()))
    if a.streams:  # 0 skips a shape
        shape("streams_x16", d_pk, off, ln, 16, cpu_us, with_rounds=True)
    del d_pk, off, ln
    if a.serial:
        d_pk, off, ln = dense_stream(a.serial, 0x5B110003)
        shape("one_stream", d_pk, off, ln, a.serial, cpu_us)
        del d_pk, off, ln
    if a.wide:
        d_pk, off, ln = dense_stream(a.wide, 0x5B110002)
        shape("wide_x1", d_pk, off, ln, 1, cpu_us)


if __name__ == "__main__":
    main()
