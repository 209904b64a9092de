"""The inputs of tests/test_gpu_long_adversarial.py (tests/long_streams.py), judged on the CPU by
the reference (oracle.unpack / oracle.decoded_size, message.zig:88-191) and by the window model,
so that the device tests cannot pass on inputs that exercise nothing: every unit's class, the
status mix, the coverage table of the window model (entry depths at X_1 and at the resolve pass's
batch edge X_32, where guessed chains meet the true one, verification rounds, output words per
window, where units end), the arithmetic that sends units to the serial decoder, and that `check`
rejects fabricated faults.

The status mix is asserted on the batch that holds every family (a family such as `cut` or
`closed` has one verdict by construction); each family's own claim is asserted per family."""
import bisect
import collections

import numpy as np
import pytest

import oracle
import long_streams as ls


def verdicts(b):
    return [ls.outcome(e, c, m) for e, c, m in zip(b.exp, b.caps, b.mis)]


def all_units():
    return [(name, u) for name in ls.FAMILIES for u in ls.family(name)]


# ---- classes -------------------------------------------------------------------------------------

def test_every_unit_has_the_class_its_family_claims():
    for name in ls.FAMILIES:
        b = ls.family_batch(name)
        assert len(b.units) == len(ls.family(name))
        for i, (u, k, c) in enumerate(zip(b.units, b.kinds, b.cls)):
            s = int(b.in_off[i]) & 15
            if name != "edge":
                assert ls.pieces(len(u), s) > ls.LONG_PIECES and len(u) >= ls.LONG_MIN, (name, k)
                assert c == ("huge" if len(u) > ls.HUGE_BYTES else "long"), (name, k)
            elif b.mis[i]:
                assert c == "other" and int(b.out_off[i]) % 8 == 4 and ls.pieces(len(u), s) > ls.LONG_PIECES
            else:
                assert k == "edge P=%d s=%d" % (len(u), s)
                assert c == ("long" if ((s + len(u) + 15) >> 4) > 320 else "other")
    e = ls.family_batch("edge")
    for s in range(16):  # both sides of the class edge at every alignment, every P in 5100 .. 5124
        mine = [(len(u), c) for u, c, o, m in zip(e.units, e.cls, e.in_off, e.mis) if int(o) & 15 == s and not m]
        assert {P for P, _ in mine} == set(range(5100, 5125)), s
        assert {c for _, c in mine} == {"long", "other"}, s
        assert (5120 - s, "other") in mine and (5121 - s, "long") in mine, s
    sizes = collections.Counter(c for name in ls.FAMILIES for c in ls.family_batch(name).cls)
    nwin = [len(u.data) / ls.WIN for _, u in all_units()]
    print("classes:", dict(sizes), "units of 33 windows and more:", sum(1 for w in nwin if w > 32))
    assert sizes["huge"] >= 2 and np.median(nwin) <= 8 and max(nwin) <= 71


def test_family_claims():
    st = {name: collections.Counter(e.st for e in ls.family_batch(name).exp) for name in ls.FAMILIES}
    print({k: dict(v) for k, v in st.items()})
    for name in ("closed", "entry", "tail", "expand"):
        assert set(st[name]) == {oracle.OK}, name
    assert set(st["random"]) == {oracle.OK, oracle.UNEXPECTED_EOF} and st["random"][oracle.OK] >= 10
    assert st["cut"][oracle.UNEXPECTED_EOF] >= len(ls.family("cut")) - 2
    assert set(st["flip"]) <= {oracle.OK, oracle.UNEXPECTED_EOF} and st["flip"][oracle.OK] >= 10
    assert st["phase"][oracle.OK] >= 10 and st["phase"][oracle.UNEXPECTED_EOF] >= 4
    assert st["edge"][oracle.UNEXPECTED_EOF] >= 60 and st["edge"][oracle.OK] >= 300
    # every phase of every pattern is a chain of its own: from any start the walk stays on it
    for pat in ls.PHASE_PATTERNS:
        body = ls.phase_body(pat, 400)
        nx, _ = ls.tables(body)
        for ph in range(len(pat)):
            r = ph
            while nx[r] != ls.EOFX and nx[r] < 300:
                r = nx[r]
                assert r % len(pat) == ph, (pat, ph)
    # flips of a tag, a 00 count and an FF count in the first, the middle and the last window, four
    # units each; cuts of four kinds in the last window of 2 .. 4 and in windows 31, 32, 33, and window 0
    kinds = collections.Counter(u.kind for u in ls.family("flip"))
    assert len(kinds) == 9 and set(kinds.values()) == {4}
    kinds = {u.kind for u in ls.family("cut")}
    assert len(kinds) == 4 * 6 + 1


def test_status_mix():
    b = ls.all_families()
    v = verdicts(b)
    cnt = collections.Counter(st for st, _ in v)
    print("all families:", len(b.units), "units,", b.in_end, "packed bytes,", b.out_end, "output bytes;", dict(cnt))
    assert cnt[oracle.OK] >= 30 and cnt[oracle.UNEXPECTED_EOF] >= 30 and cnt[oracle.OUT_OF_SPACE] >= 20
    assert cnt[oracle.INVALID_ARGUMENT] == 1
    r = ls.family_batch("random")
    assert sum(1 for e in r.exp if e.st == oracle.OK) >= 20
    assert sum(1 for st, _ in verdicts(r) if st == oracle.OK) >= 10
    # the long units share the batch with small and mid encoder output
    other = [i for i, k in enumerate(b.kinds) if k == "encoder output"]
    assert len(other) == 300 and all(b.cls[i] == "other" for i in other)
    assert min(len(b.units[i]) for i in other) <= 64 and max(len(b.units[i]) for i in other) >= 2000
    # capacities of OK units: exact, 8 B short, 24 B over, 0; failing units: a multiple of 512
    delta = collections.Counter(c - len(e.ref) for e, c, k in zip(b.exp, b.caps, b.kinds)
                                if e.st == oracle.OK and k != "edge misaligned slot")
    zero = sum(1 for e, c in zip(b.exp, b.caps) if e.st == oracle.OK and c == 0)
    assert delta[0] >= 100 and delta[-8] >= 100 and delta[24] >= 100 and zero >= 100
    assert all(c % 512 == 0 for e, c in zip(b.exp, b.caps) if e.st != oracle.OK)
    assert {int(o) & 15 for o in b.in_off} == set(range(16))
    assert all(int(o) % 8 == m for o, m in zip(b.out_off, b.mis))


# ---- the window model ----------------------------------------------------------------------------

def test_model_follows_the_reference_chain():
    """The model's wv_resolve, entered where the reference's chain enters a window, verifies for
    every lane the chain's first record start at or past the lane's chunk (EOFX past the record
    that runs over the unit's end), and leaves the window where the chain does."""
    for name, u in all_units():
        starts, eof = ls.chain(u.data)
        P = len(u.data)
        marks = starts + ([P] if eof is None else [])
        for w in ls.windows(u.data):
            if w.depth is None:
                continue
            X = w.j * ls.WIN
            Pw = min(P - X, ls.WIN)
            C = max(ls.CMIN, (Pw + 63) >> 6)
            r = w.entered
            want = [w.depth]
            for lane in range(1, ls.WAVE):
                k = bisect.bisect_left(marks, X + min(lane * C, Pw))
                want.append(marks[k] - X if k < len(marks) and (eof is None or marks[k] <= eof) else ls.EOFX)
            k = bisect.bisect_left(marks, X + Pw)
            leave = marks[k] - X if k < len(marks) else ls.EOFX
            assert list(r.ents) == want, (u.kind, w.j, [i for i in range(ls.WAVE) if r.ents[i] != want[i]][:4])
            assert r.exit == leave and (r.exit == ls.EOFX) == w.eof, (u.kind, w.j, r.exit, leave)


def coverage():
    depth = {1: set(), 32: set()}
    meet, rounds = collections.Counter(), collections.Counter()
    top = dict(rounds=0, rewalks=0, exhausted=0, words=0, big=0, nostart=0, windows=0, restage=0)
    eof_at = set()
    for name, u in all_units():
        ws = ls.windows(u.data)
        top["windows"] += len(ws)
        for w in ws:
            if w.depth is not None and w.j in depth:
                depth[w.j].add(w.depth)
            if w.j and w.depth is not None:
                m = w.meet
                meet["never" if m == ls.NEVER else "<=16" if m <= 16 else "17..72" if m <= 72 else
                     "73..144" if m <= 144 else ">144"] += 1
                top["restage"] += w.depth >= ls.WIN_D
            for r in (w.spec, w.entered):
                if r is not None:
                    rounds["0" if r.rounds == 0 else "1..2" if r.rounds <= 2 else "3..5" if r.rounds <= 5 else ">5"] += 1
                    top["rounds"] = max(top["rounds"], r.rounds)
                    top["rewalks"] = max(top["rewalks"], r.rewalks)
                    top["exhausted"] += r.exhausted
            top["words"] = max(top["words"], w.words)
            top["big"] += w.words > 32767
            if w.eof:
                eof_at.add(w.j)
                if w.j == len(ws) - 1:
                    eof_at.add("last")
        top["nostart"] += ws[-1].starts == 0 and ls.chain(u.data)[1] is None
    return depth, meet, rounds, top, eof_at


def test_coverage_table():
    depth, meet, rounds, top, eof_at = coverage()
    print("windows:", top["windows"], "meet:", dict(meet), "rounds:", dict(rounds), top,
          "EOF in windows", sorted(map(str, eof_at)))
    assert depth[1] >= set(range(73)) and depth[32] >= set(range(73))
    for k in ("<=16", "17..72", "73..144", ">144", "never"):
        assert meet[k] >= 5, k
    for k in ("0", "1..2", "3..5", ">5"):
        assert rounds[k] >= 1, k
    assert top["rounds"] <= 64
    assert top["exhausted"] >= 5 and top["rewalks"] >= 6  # a lane's seventh walk has no mark id left
    assert top["big"] >= 1 and top["nostart"] >= 1
    assert {0, 31, 32, 33, "last"} <= eof_at
    # the batch edge itself: a unit's windows 31, 32 and 33 each entered at every depth
    per = collections.defaultdict(set)
    for u in ls.family("entry"):
        ws = ls.windows(u.data)
        if len(ws) > 33:
            per[tuple(ws[j].depth for j in (31, 32, 33))].add(u.kind)
    assert {k for k in per if len(set(k)) == 1} >= {(d, d, d) for d in range(73)}


def test_serial_batch_arithmetic():
    s = ls.serial_batch()
    n = len(s.alias)
    print("serial batch:", n, "aliases of", [len(u) for u in s.units], "B;", s.windows, "windows, table",
          ls.win_cap(n), "; output", s.out_end >> 20, "MiB")
    assert s.windows > ls.win_cap(n) + 1000            # at least one unit must take the serial list
    assert s.out_end <= 512 << 20 and s.in_end <= 1 << 20
    assert all(50000 <= len(u) <= 1 << 20 for u in s.units)
    assert [e.st for e in s.exp] == [oracle.OK, oracle.OK, oracle.OK, oracle.UNEXPECTED_EOF]
    want = collections.Counter()
    for j, c in zip(s.alias, s.caps):
        want[ls.outcome(s.exp[j], int(c))[0]] += 1
    assert want[oracle.OK] >= 300 and want[oracle.OUT_OF_SPACE] == 60 and want[oracle.UNEXPECTED_EOF] == 260
    assert (np.diff(s.out_off) >= ls.FRONT + ls.BACK).all() and (s.out_off % 8 == 0).all()
    for u in s.units:  # what the serial walk does to them: the model's rounds stay in bounds
        for w in ls.windows(u):
            assert all(r is None or r.rounds <= 64 for r in (w.spec, w.entered))
    assert max(w.depth or 0 for w in ls.windows(s.units[2])) == 70  # the entry unit: depth 70 twelve times


# ---- check against fabricated device results -----------------------------------------------------

def test_check_rejects_fabricated_faults():
    b = ls.all_families()
    st, ol, out = ls.ideal(b)
    seen = ls.check(b, st, ol, out)
    assert set(seen) == {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE, oracle.INVALID_ARGUMENT}
    ls.check_sizes(b, [e.size if e.size_st == oracle.OK else 0 for e in b.exp], [e.size_st for e in b.exp])
    v = verdicts(b)
    long_ = lambda i: b.cls[i] != "other"
    i = next(k for k, (s, n) in enumerate(v) if s == oracle.OK and long_(k) and b.caps[k] > n > 0)
    j = next(k for k, (s, n) in enumerate(v) if s == oracle.UNEXPECTED_EOF and long_(k) and b.caps[k] > 0)
    t = next(k for k, (s, n) in enumerate(v) if s == oracle.OUT_OF_SPACE and long_(k) and b.caps[k] > 0)
    m = b.mis.index(4)
    o, oj, ot, om = (int(b.out_off[k]) for k in (i, j, t, m))

    def rejected(where, at=None, stat=None, length=None):
        s2, l2, o2 = st.copy(), ol.copy(), out.copy()
        if at is not None:
            o2[at] ^= 0x10
        if stat:
            s2[stat[0]] = stat[1]
        if length:
            l2[length[0]] = length[1]
        with pytest.raises(AssertionError) as info:
            ls.check(b, s2, l2, o2)
        assert where in str(info.value), (where, str(info.value))

    rejected("status", stat=(i, oracle.UNEXPECTED_EOF))          # a wrong status
    rejected("status", stat=(j, oracle.OK))
    rejected("status", stat=(t, oracle.OK))
    rejected("out_len", length=(i, v[i][1] - 8))                 # a wrong length
    rejected("out_len", length=(j, 8))
    rejected("out_len", length=(t, 0))
    rejected("decoded bytes", o)                                 # one wrong output byte
    rejected("decoded bytes", o + v[i][1] - 1)
    rejected("past out_len", o + v[i][1])                        # a byte written past out_len
    rejected("past out_len", o + b.caps[i] - 1)
    rejected("into its slot", oj)                                # a byte written into a failed slot
    rejected("into its slot", ot + b.caps[t] - 1)
    rejected("into its slot", om + 8)
    rejected("before the slot", o - 1)                           # a byte written into a guard zone
    rejected("before the slot", int(b.out_off[0]) - ls.FRONT)
    rejected("past the capacity", o + b.caps[i])
    rejected("past the capacity", out.size - 1)
    rejected("before the slot", om - 1)
    with pytest.raises(AssertionError):
        ls.check_sizes(b, [e.size + 8 for e in b.exp], [e.size_st for e in b.exp])
    # the inside of a failed slot of a unit that is not long is unspecified; its edges are not
    k = next(k for k, (s, n) in enumerate(v) if s != oracle.OK and not long_(k) and b.caps[k] > 0 and not b.mis[k])
    o2 = out.copy()
    o2[int(b.out_off[k])] ^= 0x10
    ls.check(b, st, ol, o2)
    rejected("past the capacity", int(b.out_off[k]) + b.caps[k])
