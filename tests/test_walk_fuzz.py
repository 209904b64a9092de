"""The message walker (capnp-zig_amd/csrc/kernels/message_walk.h, list_read.h) on the CPU, no GPU
needed: the headers compiled for the host (tests/host_walk) against the Python models of
struct_streams.py / list_streams.py over the generated mutants of walk_fuzz.py, at the sizes the
GPU tests use (test_gpu_walk_fuzz.py); and the conditions the generated batches have to meet
under the models alone, so that a quiet change of the generator cannot empty the GPU tests.

The host twin is loaded with ctypes as it is built: no sanitizer, nothing preloaded. The
sanitizer run is `make -C tests/host_walk asan-run`, a process of its own."""
import collections
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import list_streams as ls
import struct_streams as ss
import walk_fuzz as wf
from list_streams import LIST_POINTER, LIST_STRUCT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host_walk")
CANARY = 0xA5A5A5A5A5A5A5A5
CANARY32 = -0x5A5A5A5B

FIELD_STATUSES = {0, 8, 9, 10, 13, 15, 16, 17, 18, 20}
HEAD_STATUSES = FIELD_STATUSES | {21}
ELEMENT_STATUSES = {0, 13, 15, 16, 17, 18, 20}  # Message.init's and the head's own are the head's


# ---------------------------------------------------------------------------
# the batches and the models' answers, computed once
# ---------------------------------------------------------------------------
class Cases:
    def __init__(self):
        ss.SEEN.clear()
        self.fields = wf.fields_batch()
        self.fields_want, self.fields_high = wf.model_fields(self.fields, ss.FIELDS)
        self.sweep = wf.sweep_batch()
        self.sweep_tables = wf.sweep_tables()
        self.sweep_want = [wf.model_fields(self.sweep, t)[0] for t in self.sweep_tables]
        # 8,000 more mutants for the twin alone, under one more random table of 32 fields
        self.extra = wf.Batch(wf.mutants(8000, "both", seed=8, cut=1 / 7))
        self.extra_table = wf.random_fields(wf.table_rng(8), 32)
        self.extra_want = wf.model_fields(self.extra, self.extra_table)[0]
        self.lists = wf.list_batch()
        self.small = self.lists.head(1000)
        self.runs = []  # (run, fields, batch, want, high)
        for run in ls.RUNS:
            batch = self.lists if run in ls.RUNS[:4] else self.small
            for fields in wf.run_tables(run):
                want, high = wf.model_lists(batch, run[0], run[1], fields, run[2])
                self.runs.append((run, fields, batch, want, high))
        # the struct-of-one-pointer reading of a slot is the restated list readers' (as
        # test_list_streams.py asserts on the corpus), here on the mutants
        for run, fields, batch, want, high in self.runs:
            if run[0] == LIST_POINTER and fields is ls.POINTER_FIELDS and run in ls.RUNS[:4]:
                for data, off, (head, rows) in list(zip(batch.msgs, batch.offs, want))[:1000]:
                    if head.status == ss.OK and rows:
                        m = ss.Msg(data)
                        lst = (head.segment, head.elems_off - off - m.starts[head.segment], head.count, 0, 1)
                        for k, row in enumerate(rows):
                            assert row == [ls.reader_field(m, lst, k, f, off) for f in fields]
        self.seen = set(ss.SEEN)


@pytest.fixture(scope="module")
def cases():
    return Cases()


def histogram(rows):
    return collections.Counter(r[0] for row in rows for r in row)


def test_batches_are_more_than_one_block_with_a_partial_last_one(cases):
    assert 7900 <= cases.fields.n <= 8500 and cases.fields.n % 256
    assert cases.sweep.n == 515 and len(cases.sweep_tables) == 32
    assert [len(t) for t in cases.sweep_tables] == list(range(1, 33))
    assert 3000 <= cases.lists.n <= 3500 and cases.lists.n % 256 and cases.small.n == 1000


def test_read_fields_batch_reaches_every_status(cases):
    h = histogram(cases.fields_want)
    assert set(h) == FIELD_STATUSES and min(h.values()) >= 32, sorted(h.items())
    assert .25 <= h[0] / sum(h.values()) <= .75
    pooled = sum((histogram(w) for w in cases.sweep_want), collections.Counter())
    assert set(pooled) == FIELD_STATUSES and min(pooled.values()) >= 32, sorted(pooled.items())
    assert .25 <= pooled[0] / sum(pooled.values()) <= .75


def test_list_calls_reach_every_status(cases):
    heads, elements = collections.Counter(), collections.Counter()
    for run, fields, batch, want, high in cases.runs:
        heads.update(h.status for h, rows in want)
        for h, rows in want:
            elements.update(histogram(rows))
        if run in ls.RUNS[:4]:  # each of the runs that read a list: thousands of elements, good heads and failing ones
            mine = collections.Counter(h.status for h, rows in want)
            assert sum(h.count for h, rows in want) > 4000 and mine[0] > 1000 and len(mine) >= 9, (run, mine)
    assert set(heads) == HEAD_STATUSES and min(heads.values()) >= 32, sorted(heads.items())
    assert set(elements) == ELEMENT_STATUSES and min(elements.values()) >= 32, sorted(elements.items())
    assert .25 <= heads[0] / sum(heads.values()) <= .75, sorted(heads.items())
    assert .25 <= elements[0] / sum(elements.values()) <= .75, sorted(elements.items())
    struct_heads = collections.Counter(h.status for run, f, b, want, high in cases.runs if run[0] == LIST_STRUCT
                                       for h, rows in want)
    assert struct_heads[ls.INVALID_INLINE_COMPOSITE_POINTER] >= 32


def test_both_ways_of_every_check_of_the_models(cases):
    missing = [(c, way) for c in ls.CHECKS + ss.CHECKS for way in (False, True) if (c, way) not in cases.seen]
    assert not missing, missing
    assert ("sget.bounds", True) not in cases.seen


def test_segments_on_both_sides_of_kSrSegs(cases):
    """a tenth of the messages and more look a segment at or past kSrSegs = 4 up (MwSegsLds's and
    MwSegsHead's table walks), and the rest stay below it"""
    flags = [cases.fields_high] + [high for run, f, b, want, high in cases.runs if run in ls.RUNS[:4]]
    for high in flags:
        assert .10 <= sum(high) / len(high) <= .60
    # messages of exactly kSrSegs segments and of one more, among those that pass Message.init
    counts = collections.Counter(int.from_bytes(m[:4], "little") + 1 for m in cases.fields.msgs if len(m) >= 8)
    assert all(counts[k] > 300 for k in wf.NSEGS), counts


def test_the_model_raises_nothing_but_its_own_errors():
    """harder damage than the batches': up to six mutations a message, cuts among them, under
    random tables and every list run"""
    rng = np.random.default_rng([wf.SEED, 6])
    tables = wf.sweep_tables()
    for j in range(300):
        data, about = (wf.struct_base if j % 2 else wf.list_base)(rng)
        words = wf.read_words(data, about["schema"])
        for k in range(6):
            m = data
            for _ in range(int(rng.integers(1, 4))):
                m = wf.mutate(rng, m, words, cut=.15) if len(m) >= 16 and ok_header(m) else m
            ss.read_fields(m, tables[(j + k) % 32])
            for kind, index, path in ls.RUNS:
                ls.read_list(m, kind, index, ls.fields_of(kind), path, limit=200)


def ok_header(m):
    """mutate() parses the table of the message it damages: only messages whose table is whole"""
    try:
        ss.Msg(m)
        return True
    except ss.RefError:
        return False


# ---------------------------------------------------------------------------
# the host twin
# ---------------------------------------------------------------------------
def test_stub_helpers_are_the_real_header_s_text():
    """stubs/kernels/device_helpers.h restates gload64 and ptr_offset_words: character for character"""
    with open(os.path.join(ROOT, "capnp-zig_amd", "csrc", "kernels", "device_helpers.h")) as f:
        real = f.read()
    with open(os.path.join(HOST, "stubs", "kernels", "device_helpers.h")) as f:
        stub = f.read()
    for name in ("gload64", "ptr_offset_words"):
        pattern = re.compile(r"^__device__ __forceinline__ \w+ " + name + r"\(.*?^}\n", re.M | re.S)
        a, b = pattern.findall(real), pattern.findall(stub)
        assert len(a) == 1 and a == b, name
    # and nothing else in the stub is code: the two functions are its whole namespace
    body = stub[stub.index("namespace cpk {") + len("namespace cpk {"):stub.index("}  // namespace cpk")]
    for name in ("gload64", "ptr_offset_words"):
        body = re.sub(r"^__device__ __forceinline__ \w+ " + name + r"\(.*?^}\n", "", body, flags=re.M | re.S)
    assert not body.strip()


def u64(values):
    return np.ascontiguousarray(np.asarray(values, dtype=np.uint64))


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Twin:
    def __init__(self, out):
        self.out = out
        self.lib = ctypes.CDLL(os.path.join(out, "libwalk_host.so"))
        for name in ("walk_read_fields", "walk_list_heads", "walk_read_elements"):
            getattr(self.lib, name).restype = None
        assert not os.environ.get("LD_PRELOAD"), "the twin is compared as built: nothing preloaded"

    def read_fields(self, batch, fields):
        """-> [4, n_fields, n] uint64: status, value, len, count"""
        n, nf = batch.n, len(fields)
        buf = np.frombuffer(batch.buf, dtype=np.uint8)
        out = np.full((3, nf * n + 2), CANARY, dtype=np.uint64)
        st = np.full(nf * n + 2, CANARY32, dtype=np.int32)
        table = np.frombuffer(wf.pack_fields(fields), dtype=np.uint8)
        self.lib.walk_read_fields(ptr(buf), ptr(u64(batch.offs)), ptr(u64(batch.lens)), ctypes.c_uint32(n), ptr(table),
                                  ctypes.c_uint32(nf), ptr(out[0][1:]), ptr(out[1][1:]), ptr(out[2][1:]), ptr(st[1:]))
        assert (out[:, 0] == CANARY).all() and (out[:, -1] == CANARY).all() and st[0] == st[-1] == CANARY32
        assert (st[1:-1] != CANARY32).all(), "a result was not written"
        return np.stack([st[1:-1].astype(np.uint64).reshape(nf, n)] + [o[1:-1].reshape(nf, n) for o in out])

    def chain(self, batch, kind, index, path, fields, cap=None):
        """heads -> a scan of the counts -> elements: (heads, start, parent, index, [4, n_fields, cap])"""
        n, nf = batch.n, len(fields)
        buf = np.frombuffer(batch.buf, dtype=np.uint8)
        offs, lens = u64(batch.offs), u64(batch.lens)
        head = np.full(32 * (n + 2), 0xA5, dtype=np.uint8)
        count = np.full(n + 2, CANARY, dtype=np.uint64)
        hst = np.full(n + 2, CANARY32, dtype=np.int32)
        p = np.asarray(tuple(path) + (0,) * 4, dtype=np.uint32)
        self.lib.walk_list_heads(ptr(buf), ptr(offs), ptr(lens), ctypes.c_uint32(n), ptr(p), ctypes.c_uint32(len(path)),
                                 ctypes.c_uint32(index), ctypes.c_uint32(kind), ptr(head[32:]), ptr(count[1:]),
                                 ptr(hst[1:]))
        assert (head[:32] == 0xA5).all() and (head[-32:] == 0xA5).all()
        assert count[0] == count[-1] == CANARY and hst[0] == hst[-1] == CANARY32
        heads = head[32:-32].view(wf.ls_head_dtype())
        assert (heads["status"] == hst[1:-1]).all() and (heads["count"] == count[1:-1]).all()
        start = np.concatenate([[0], np.cumsum(count[1:-1])]).astype(np.uint64)
        total = int(start[-1])
        cap = total if cap is None else cap
        rows = min(total, cap)
        out = np.full((3, nf * cap + 2), CANARY, dtype=np.uint64)
        st = np.full(nf * cap + 2, CANARY32, dtype=np.int32)
        num = np.full((2, cap + 2), 0xA5A5A5A5, dtype=np.uint32)
        table = np.frombuffer(wf.pack_fields(fields), dtype=np.uint8)
        if cap:
            self.lib.walk_read_elements(ptr(buf), ptr(offs), ctypes.c_uint32(n), ptr(head[32:]), ptr(start),
                                        ctypes.c_uint32(kind), ctypes.c_uint64(cap), ptr(table), ctypes.c_uint32(nf),
                                        ptr(num[0][1:]), ptr(num[1][1:]), ptr(out[0][1:]), ptr(out[1][1:]),
                                        ptr(out[2][1:]), ptr(st[1:]))
        assert (out[:, 0] == CANARY).all() and (out[:, -1] == CANARY).all() and st[0] == st[-1] == CANARY32
        shape = (nf, cap)
        res = np.stack([st[1:-1].astype(np.int64).astype(np.uint64).reshape(shape)] + [o[1:-1].reshape(shape) for o in out])
        assert (st[1:-1].reshape(shape)[:, rows:] == CANARY32).all() and (res[1:, :, rows:] == CANARY).all()
        assert (num[:, 1 + rows:] == 0xA5A5A5A5).all()
        return heads, start, num[0][1:1 + rows], num[1][1:1 + rows], res[:, :, :rows]


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None or shutil.which("make") is None:
        pytest.skip("no host C++ compiler (or no make) on this machine")
    out = str(tmp_path_factory.mktemp("host_walk"))
    run = subprocess.run(["make", "-s", "-C", HOST, "OUT=" + out, "CXX=" + cxx, "all"], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    return Twin(out)


def expect_fields(want):
    """want[i][f] -> [4, n_fields, n] uint64"""
    return np.ascontiguousarray(np.array(want, dtype=np.uint64).transpose(2, 1, 0))


def assert_fields(got, want, fields, what):
    exp = expect_fields(want)
    bad = np.argwhere(got != exp)
    if len(bad):
        j, f, i = bad[0]
        raise AssertionError(f"{what}: {len(bad)} differ; first: {('status', 'value', 'len', 'count')[j]} of field {f} "
                             f"({fields[f]}) of unit {i}: {got[:, f, i].tolist()} != {exp[:, f, i].tolist()}")


def test_twin_read_fields_fixed_table(cases, twin):
    assert_fields(twin.read_fields(cases.fields, ss.FIELDS), cases.fields_want, ss.FIELDS, "read_fields")


def test_twin_read_fields_more_mutants_a_seventh_of_them_cut(cases, twin):
    assert cases.fields.n + cases.sweep.n + cases.lists.n + cases.extra.n >= 20000
    assert_fields(twin.read_fields(cases.extra, cases.extra_table), cases.extra_want, cases.extra_table, "extra")


def test_twin_read_fields_swept_tables(cases, twin):
    for table, want in zip(cases.sweep_tables, cases.sweep_want):
        assert_fields(twin.read_fields(cases.sweep, table), want, table, f"{len(table)} fields")


def assert_chain(got, want, fields, cap, what):
    heads, start, parent, index, res = got
    n = len(want)
    mine = [wf.head_tuple(h) for h in heads]
    theirs = [w[0].tuple() for w in want]
    bad = [i for i in range(n) if mine[i] != theirs[i]]
    assert not bad, f"{what}: head of unit {bad[0]}: {mine[bad[0]]} != {theirs[bad[0]]} ({len(bad)} differ)"
    counts = [w[0].count for w in want]
    assert start.tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    rows = min(int(start[-1]), cap if cap is not None else int(start[-1]))
    assert parent.tolist() == np.repeat(np.arange(n), counts)[:rows].tolist()
    assert index.tolist() == np.concatenate([np.arange(c) for c in counts] + [np.zeros(0, dtype=np.int64)])[:rows].tolist()
    flat = [row for h, r in want for row in r][:rows]
    assert len(flat) == rows
    if rows and fields:
        exp = expect_fields(flat)
        bad = np.argwhere(res != exp)
        if len(bad):
            j, f, e = bad[0]
            raise AssertionError(f"{what}: {len(bad)} differ; first: {('status', 'value', 'len', 'count')[j]} of field "
                                 f"{f} ({fields[f]}) of element {e} (unit {parent[e]}, element {index[e]}): "
                                 f"{res[:, f, e].tolist()} != {exp[:, f, e].tolist()}")


def test_twin_lists(cases, twin):
    for run, fields, batch, want, high in cases.runs:
        got = twin.chain(batch, run[0], run[1], run[2], fields)
        assert_chain(got, want, fields, None, f"run {run}")


def test_twin_lists_with_half_the_capacity(cases, twin):
    run, fields, batch, want, high = cases.runs[0]
    cap = sum(h.count for h, rows in want) // 2 + 1
    assert_chain(twin.chain(batch, run[0], run[1], run[2], fields, cap=cap), want, fields, cap, "half the capacity")


def test_the_program_answers_as_the_model_does(cases, twin, tmp_path):
    """walk_fuzz_main (the program `make asan-run` builds with the sanitizers) on 600 mutants, each
    in a heap block of exactly its length, against the models at base 0"""
    msgs = cases.fields.msgs[:300] + cases.lists.msgs[:300]
    runs = wf.program_runs()
    units, tables, out = (str(tmp_path / name) for name in ("units.bin", "tables.bin", "results.bin"))
    wf.write_units(units, msgs)
    wf.write_tables(tables, ss.FIELDS, runs)
    done = subprocess.run([os.path.join(twin.out, "walk_fuzz_main"), units, tables, out], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert f"{len(msgs)} units, {len(runs)} list runs" in done.stdout and "field statuses: 0=" in done.stdout
    got_fields, got_runs = wf.read_results(out, len(msgs), ss.FIELDS, runs)
    for i, m in enumerate(msgs):
        assert [tuple(r) for r in got_fields[i]] == ss.read_fields(m, ss.FIELDS), i
    for (kind, index, path, fields), per in zip(runs, got_runs):
        for i, m in enumerate(msgs):
            head, rows = ls.read_list(m, kind, index, fields, path, limit=wf.ELEM_LIMIT)
            assert wf.head_tuple(per[i][0]) == head.tuple(), (kind, index, path, i)
            assert [[tuple(r) for r in row] for row in per[i][1]] == rows, (kind, index, path, i)
