"""read_fields_batch, list_heads_batch and read_elements_batch on the device over the generated
mutants of walk_fuzz.py, against the Python models. What the host twin
of test_walk_fuzz.py cannot show is here: 256 lanes side by side in the LDS columns of the segment
bounds and of the staged results, every lane of a wave on another message shape and another
outcome, and read_elements_kernel's block-cooperative parent lookup over lists of 0..17 elements.

Messages lie back to back between fillers of distinct nonzero bytes (struct_streams.layout) and
every output has canaries on both sides, as in test_gpu_read_fields.py / test_gpu_read_lists.py.
The batches are the smallest that hold all of it: more than one block, a partial last block,
segment counts on both sides of kSrSegs, all residues of n_fields modulo kSrGroup."""
import numpy as np
import pytest

import list_streams as ls
import struct_streams as ss
import walk_fuzz as wf
from test_gpu_read_fields import Read
from test_gpu_read_lists import Chain, dev_bytes, model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def check_read(r, want):
    """Read.check, vectorised: want[i][f] = (status, value, len, count)"""
    st, v, l, c = r.results()
    exp = np.array(want, dtype=np.uint64).transpose(2, 1, 0)  # [4, n_fields, n]
    got = [st.astype(np.int64).astype(np.uint64), v, l] + ([c] if r.with_count else [])
    for j, (name, g) in enumerate(zip(("status", "value", "len", "count"), got)):
        bad = np.argwhere(g != exp[j])
        assert not len(bad), (f"{len(bad)} differ; first: {name} of field {bad[0][0]} ({r.fields[bad[0][0]]}) of message "
                              f"{bad[0][1]}: {g[tuple(bad[0])]} != {exp[j][tuple(bad[0])]}")


# ---- read_fields_batch ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixed():
    b = wf.fields_batch()
    return b, dev_bytes(b.buf), wf.model_fields(b, ss.FIELDS)[0]


@pytest.mark.parametrize("with_count", [True, False], ids=["count", "count-null"])
def test_read_fields_fixed_table(fixed, with_count):
    """about 8,000 mutants in shuffled order, one launch: failing and good lanes share every wave"""
    b, d_in, want = fixed
    assert b.n % 256
    check_read(Read(d_in, b.offs, b.lens, ss.FIELDS, with_count=with_count), want)


@pytest.fixture(scope="module")
def sweep():
    b = wf.sweep_batch()
    return b, dev_bytes(b.buf), wf.sweep_tables()


@pytest.mark.parametrize("n_fields", range(1, 33))
def test_read_fields_swept_tables(sweep, n_fields):
    """one random table of each length over 515 mutants: every residue of kSrGroup and its last
    flush, paths in any order, the `same` bit set and clear"""
    b, d_in, tables = sweep
    table = tables[n_fields - 1]
    assert len(table) == n_fields and b.n == 515
    check_read(Read(d_in, b.offs, b.lens, table), wf.model_fields(b, table)[0])


# ---- list_heads_batch -> lengths_to_offsets -> read_elements_batch ---------------------------------
@pytest.fixture(scope="module")
def lists():
    b = wf.list_batch()
    small = b.head(1000)
    return (b, dev_bytes(b.buf)), (small, dev_bytes(small.buf))


CASES = [(run, t) for run in ls.RUNS for t in range(len(wf.run_tables(run)))]


@pytest.mark.parametrize("run,table", CASES, ids=[
    f"{'struct' if r[0] == ls.LIST_STRUCT else 'pointer'}-{r[1]}-{r[2]}-{'random' if t else 'schema'}" for r, t in CASES])
def test_lists(lists, run, table):
    """about 3,000 list-schema mutants for a run that reads a list as what it is (with its
    schema's table and with a random one), 1,000 for the others; elem_cap is the model's total
    (1 where no list resolves: the one row stays unwritten)"""
    b, d_in = lists[0] if run in ls.RUNS[:4] else lists[1]
    kind, index, path = run
    fields = wf.run_tables(run)[table]
    want = model(b.msgs, b.offs, kind, index, fields, path)
    total = sum(h.count for h, rows in want)
    r = Chain(d_in, b.offs, b.lens, kind, index, fields, path, elem_cap=max(total, 1)).check(want)
    assert int(r["start"][-1]) == total


def test_lists_with_half_the_capacity(lists):
    b, d_in = lists[0]
    kind, index, path = ls.RUNS[0]
    fields = ls.fields_of(kind)
    total = sum(ls.read_list(m, kind, index, [], path, limit=0)[0].count for m in b.msgs)
    cap = total // 2 + 1
    r = Chain(d_in, b.offs, b.lens, kind, index, fields, path, elem_cap=cap).check(
        model(b.msgs, b.offs, kind, index, fields, path, cap=cap))
    assert int(r["start"][-1]) == total > cap
