"""read_message_batch on the reader-stream corpus (tests/reader_streams.py: about 6,000 streams
around the framed-length cut, tests/test_reader_streams.py holds its coverage table), against
oracle_read_packed_message, unit by unit.

Unlike gpu_read (test_gpu_read_message.py) the streams lie densely at random byte alignments,
all 16 of them in one launch, and the slots are 8-B aligned at every phase of a 128-B line with
64 canary bytes on both sides, as in test_gpu_words_adversarial.py for the decoder. Caps cycle
over the exact framed length, + 24, 9000 (walk route: framed + 4096) and, for streams the oracle
reads OK, 8 bytes short (OUT_OF_SPACE with the framed length and the packed length). Checks:
status, framed bytes and consumed equal the oracle's; errors leave out_len = consumed = 0
(include/capnp_packed.h); nothing is written before a slot or from out_off + cap on, for any
status, nor in [out_len, cap) for OK units. A failed unit may leave anything inside its slot
(the default contract).
"""
import collections

import numpy as np
import pytest

import capnp_packed as cp
import reader_streams as rs
from test_gpu_read_message import ORACLE_TO_ABI

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"

# status name -> C-ABI status, through test_gpu_read_message.py's oracle code -> C-ABI map
CODES = {rs.ORACLE_NAME[rc]: abi for rc, abi in ORACLE_TO_ABI.items()}
CODES["OUT_OF_SPACE"] = cp.OUT_OF_SPACE


def launch(buf, in_off, in_len, out_bytes, out_off, caps):
    """One read_message_batch over a canary-filled output and junk-filled result arrays."""
    n = len(in_off)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)
    d_in = buf if isinstance(buf, torch.Tensor) else torch.from_numpy(buf).to(DEV)
    d_out = torch.full((out_bytes,), rs.SENT, dtype=torch.uint8, device=DEV)
    out_len = torch.full((n,), 7, dtype=torch.int64, device=DEV)
    used = torch.full((n,), 7, dtype=torch.int64, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.read_message_batch(d_in, t(in_off), t(in_len), d_out, t(out_off), t(caps), out_len, used, status)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_len.cpu().numpy(), used.cpu().numpy(), status.cpu().numpy()


def read_and_compare(rng, cs, first_cap=0):
    """Lay the cases out, read them in one launch, compare: (mismatches, layout, results)."""
    caps = rs.choose_caps(cs, first_cap)
    buf, in_off, out_off, out_bytes = rs.layout(rng, cs, caps)
    out, ol, used, st = launch(buf, in_off, [len(c.data) for c in cs], out_bytes, out_off, caps)
    bad = rs.compare(cs, caps, out_off, out, ol, used, st, CODES)
    return bad, (buf, in_off, out_off, caps), (ol, used, st)


def report(cs, bad):
    return [(i, cs[i].family, cs[i].fw, len(cs[i].data), cs[i].status) + tuple(rest) for i, *rest in bad[:12]]


@pytest.fixture(scope="module")
def cases():
    return rs.cases(rs.SEED)


@pytest.fixture(scope="module")
def whole(cases):
    """The whole corpus in one launch, in shuffled order: words-route, walk-route and
    header-error units share waves."""
    rng = np.random.default_rng(0xF00D)
    cs = [cases[i] for i in rng.permutation(len(cases))]
    bad, lay, res = read_and_compare(rng, cs)
    return cs, bad, lay, res


def test_whole_corpus_in_one_launch(whole):
    cs, bad, (buf, in_off, out_off, caps), (ol, used, st) = whole
    # every stream alignment and every slot phase, in each words-route outcome
    a_in, a_out = collections.defaultdict(set), collections.defaultdict(set)
    for c, i, o in zip(cs, in_off, out_off):
        if c.fw is not None and c.fw <= rs.WORDS_ROUTE_MAX and rs.outcome(c) in rs.OUTCOMES:
            a_in[rs.outcome(c)].add(int(i) & 15)
            a_out[rs.outcome(c)].add((int(o) >> 3) & 15)
    for kind in rs.OUTCOMES:
        assert a_in[kind] == set(range(16)) and a_out[kind] == set(range(16)), kind
    seen = collections.Counter(int(x) for x in st)
    for code in CODES.values():
        assert seen[code] > 0, code
    assert not bad, (len(bad), report(cs, bad))


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 129])
def test_words_route_alone_in_partial_waves(cases, batch):
    """The words-route streams alone (no walk pass, no header error in the launch), in launches
    of 1, 63, 64, 65 and 129 units: partial waves and the 2-wave block. Each size takes every
    fifth stream from its own start (single-unit launches: 192 of those, a launch each)."""
    sizes = [1, 63, 64, 65, 129]
    rng = np.random.default_rng(0xBA7C + batch)
    sub = [c for c in cases if c.fw is not None and c.fw <= rs.WORDS_ROUTE_MAX][sizes.index(batch)::5]
    sub = [sub[i] for i in rng.permutation(len(sub))][:192 if batch == 1 else None]
    kinds = set()
    for lo in range(0, len(sub), batch):
        cs = sub[lo:lo + batch]
        bad, _, _ = read_and_compare(rng, cs, first_cap=lo // batch)
        assert not bad, (lo, len(bad), report(cs, bad))
        kinds |= {rs.outcome(c) for c in cs}
    assert kinds >= set(rs.OUTCOMES)


def test_message_by_message(whole):
    """The socket-reader loop: every OK unit whose stream holds a complete next message is read
    again from in_off + consumed, in place, and must return that message: a second check of
    consumed (the kernel rebuilds it from a ring offset and a count of 64-B rounds), and reads
    that start inside another unit's stream."""
    cs, bad, (buf, in_off, out_off, caps), (ol, used, st) = whole
    assert not bad, "the first read failed (test_whole_corpus_in_one_launch)"
    nxt, offs = [], []
    for i, c in enumerate(cs):
        if c.status != rs.OK or st[i] != cp.OK:
            continue
        rest = c.data[int(used[i]):]
        status, framed, consumed = rs.oracle_read(rest)
        if status == rs.OK:
            h = rs.read_message(rest, header_only=True)
            nxt.append(rs.Case(rest, "exact", None, None, status, framed, consumed, h.fw, h.spans))
            offs.append(int(in_off[i]) + int(used[i]))
    assert len(nxt) >= 64
    assert any(len(c.framed) > 4096 for c in nxt) and any(o & 15 for o in offs)
    rng = np.random.default_rng(0x2E57)
    caps2 = rs.choose_caps(nxt)
    _, _, out_off2, out_bytes2 = rs.layout(rng, nxt, caps2)
    out, ol2, used2, st2 = launch(buf, offs, [len(c.data) for c in nxt], out_bytes2, out_off2, caps2)
    bad2 = rs.compare(nxt, caps2, out_off2, out, ol2, used2, st2, CODES)
    assert not bad2, (len(bad2), report(nxt, bad2))
