"""The build plan on the host (tests/host_build/): the plain build of the
stand-alone program runs capnp-zig_amd/csrc/build_plan.h's plan compiler and layout function (the
text the kernel compiles) over the model's corpus and over failing columns, and its acceptance,
statuses and sizes are the model's. The program's own invariants (allocations disjoint, in op
order, summing to the total) are asserted inside it; `make -C tests/host_build asan-run` runs its
generated programs under ASan + UBSan."""
import os
import random
import shutil
import subprocess

import pytest

import build_streams as bs
from build_streams import Op

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_build")
S = bs.STRUCT


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("make") is None or shutil.which(os.environ.get("CXX", "c++")) is None:
        pytest.skip("no C++ toolchain on this machine")
    out = str(tmp_path_factory.mktemp("host_build"))
    subprocess.run(["make", "-s", "-C", HERE, "OUT=" + out, "all"], check=True)
    return os.path.join(out, "build_host_main")


def cases():
    """[(ops, pool_len, [cols])]: the corpus, then rows that fail each slice check, then refused programs"""
    out = []
    for ops, rows in bs.corpus():
        pool, cols = bs.columns(ops, rows)
        out.append((ops, len(pool), cols))
    ops = [Op(S, dw=1, pw=4), Op(bs.LIST_16, 0), Op(bs.LIST_BIT, 1), Op(bs.DATA, 2), Op(bs.TEXT, 3), Op(bs.U8, 0)]
    good = [(0, 0, 0), (0, 4, 0), (4, 2, 9), (8, 5, 0), (1, 3, 0), (7, 0, 0)]
    rows = [good]
    for k, entry in [(1, (0, 3, 0)), (2, (4, 1, 9)), (2, (4, 2, 17)), (3, (0, 1 << 29, 0)), (3, (60, 5, 0)),
                     (3, (65, 0, 0)), (3, (64, 0, 0)), (4, (0, (1 << 29) - 1, 0)), (4, (0, (1 << 29) - 2, 0)),
                     (4, (0, bs.ABSENT - 1, 0)), (1, (0, bs.ABSENT, 0)), (2, (0, 0, bs.ABSENT)),
                     (3, (1 << 63, 1 << 63, 0)), (1, (1 << 40, 6, 0))]:
        rows.append(good[:k] + [entry] + good[k + 1:])
    out.append((ops, 64, rows))
    out.append((ops, 1 << 30, rows))
    rng = random.Random(5)
    for _ in range(60):  # programs broken in one place: mostly refused
        ops = bs.gen_program(rng, rng.randrange(2, 20))
        o = ops[rng.randrange(1, len(ops))]
        what = rng.randrange(5)
        if what == 0:
            o.target = rng.randrange(len(ops) + 1)
        elif what == 1:
            o.offset = rng.randrange(8)
        elif what == 2:
            o.bit = rng.randrange(9)
        elif what == 3:
            o.kind = rng.randrange(20)
        else:
            o.reserved = (0, 0, 1)
        out.append((ops, 0, []))
    return out


def test_plan_and_layout_agree_with_the_model(program, tmp_path):
    cs = cases()
    lines = []
    for ops, pool_len, cols in cs:
        lines.append(f"{len(ops)} {pool_len}")
        lines += [f"{o.kind} {o.target} {o.offset} {o.bit} {o.dw} {o.pw} {o.reserved[2]}" for o in ops]
        lines.append(str(len(cols)))
        lines += [" ".join(str(x) for entry in col for x in entry) for col in cols]
    src, dst = tmp_path / "cases.txt", tmp_path / "layout.txt"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([program, str(src), str(dst)], check=True)
    got = dst.read_text().split("\n")
    at, statuses, refused = 0, set(), 0
    for ops, pool_len, cols in cs:
        head = got[at]
        at += 1
        if not bs.check_ops(ops):
            assert head == "refused", ops
            refused += 1
            continue
        assert head == f"accepted {1 + sum(o.dw + o.pw for o in ops if o.kind == S)}", ops
        for col in cols:
            st, framed, _ = bs.build_message(ops, col, b"", pool_len=pool_len, sizes_only=True)
            if st == bs.MESSAGE_TOO_LARGE:  # the kernel's check on the layout's total, not the layout's
                st, framed = bs.OK, None
            fields = [int(x) for x in got[at].split()]
            at += 1
            statuses.add(st)
            assert fields[0] == st, (ops, col)
            if st == bs.OK and framed is not None:
                assert 8 * (fields[1] + 1) == framed
                assert len(fields) == 2 + len(ops) and fields[2] == 1 and sorted(fields[2:]) == fields[2:]
    assert got[at:] == [""]
    assert statuses == {bs.OK, bs.INVALID_ARGUMENT, bs.LIST_TOO_LARGE, bs.OUT_OF_BOUNDS} and refused > 20
