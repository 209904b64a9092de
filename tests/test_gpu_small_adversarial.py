"""The small-unit decoders (decode_small_kernel, and decode_small_group_kernel under
capnp_packed_set_all_or_nothing(1)) on adversarial and class-edge input, unit by
unit and bit for bit against the oracle's unpackPacked / estimateUnpackedSize
(message.zig:88-191). The inputs are tests/small_streams.py's, judged on the CPU by
tests/test_small_streams.py: small units of 161 .. 512 packed bytes of every kind (random bytes,
record streams with 00 counts up to 255 and literal words holding zero bytes, C++-dialect
streams, one replaced tag or count, cut tails, 00 FF chains), a tag, count and literal word
start at every offset of a lane's 64-B ring, packed streams at every `address & 15`, slots at
every 8-B phase of a 64-B chunk with 64 canary bytes on both sides, and capacities around the
decoded size that are no multiple of 8.
- corpus parity, alone and with mid and long units between the small ones;
- partial waves (1, 63, 64, 65, 257 units) with misaligned slots;
- 2^20 units, four times the lane kernel's resident grid: lanes take second and later units, and
  cached blocks of 64 list entries are refilled, beside units that fail;
- the class-edge lattice: exact packed lengths on every class bound, slots around every bound;
- hand-built sequences that make the group kernel cut a group by its piece sum and by its
  capacity-word sum.
Every test runs decoded_size_batch on the same units, and (but for the last) runs under both
small-unit decoders; a failed unit's slot stays untouched wherever the contract says so."""
import contextlib

import numpy as np
import pytest

import capnp_packed as cp
import oracle
import small_streams as ss

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"

both_small_decoders = pytest.mark.parametrize("aon", [False, True], ids=["lane", "group"])


@contextlib.contextmanager
def all_or_nothing(on):
    prev = cp.set_all_or_nothing(on)
    try:
        yield
    finally:
        cp.set_all_or_nothing(prev)


def run_arrays(d_in, in_off, in_len, out_bytes, out_off, caps):
    """decode_batch into a buffer of SENT, and decoded_size_batch, of the same units."""
    n = len(in_off)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)  # noqa: E731
    d_out = torch.full((out_bytes,), ss.SENT, dtype=torch.uint8, device=DEV)
    out_len = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    sz_len = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    sz_st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_off, d_len = t(in_off), t(in_len)
    cp.decode_batch(d_in, d_off, d_len, d_out, t(out_off), t(caps), out_len, status)
    cp.decoded_size_batch(d_in, d_off, d_len, sz_len, sz_st)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy(), sz_len.cpu().numpy(), sz_st.cpu().numpy()


def run(b):
    d_in = torch.from_numpy(ss.packed_stream(b.units, b.in_off, b.in_end)).to(DEV)
    return run_arrays(d_in, b.in_off, [len(u) for u in b.units], b.out_end + ss.BACK, b.out_off, b.caps)


def untouched_on_failure(b, aon, decoder):
    """Per unit: must a failed unit leave its whole slot untouched? Always under all-or-nothing
    (which also sends the mid units to the two-pass decoder) and for long units; otherwise a small
    unit may keep a prefix of its words, and so may a mid unit unless the two-pass decoder is forced."""
    out = []
    for i, u in enumerate(b.units):
        long_ = not ss.is_small(b, i) and ss.pieces(u, int(b.in_off[i]) & 15) > ss.LONG_PIECES
        out.append(aon or long_ or (not ss.is_small(b, i) and decoder == "twopass"))
    return out


def decode_and_check(b, aon, decoder=None):
    with all_or_nothing(aon):
        out, ol, st, sz_len, sz_st = run(b)
    seen = ss.check(b, out, st, ol, untouched_on_failure(b, aon, decoder))
    ss.check_sizes(b, sz_len, sz_st)
    return seen


# ---- a. corpus parity ---------------------------------------------------------------------

@both_small_decoders
def test_corpus_parity(aon):
    seen = decode_and_check(ss.main_corpus(), aon)
    assert seen == {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE}


@both_small_decoders
def test_corpus_parity_between_mid_and_long_units(decoder, aon):
    """Every third unit is a mid unit (600 .. 3000 packed bytes) or, six times, a long one, so the
    small list is not the identity and the three classes' kernels run side by side."""
    seen = decode_and_check(ss.mixed_corpus(), aon, decoder)
    assert seen == {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE}


# ---- b. partial waves ---------------------------------------------------------------------

@both_small_decoders
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_partial_waves(n, aon):
    """Batches that end inside a wave's first 64 entries, on them, one past them, and one past a
    block; an empty unit on a misaligned slot is OK with nothing written, a non-empty one
    INVALID_ARGUMENT."""
    if n == 1:
        for b in ss.single_units():
            decode_and_check(b, aon)
        return
    seen = decode_and_check(ss.partial_wave(n), aon)
    assert oracle.INVALID_ARGUMENT in seen and oracle.OK in seen


# ---- c. lane refill past the resident grid ------------------------------------------------

@both_small_decoders
def test_lane_refill_past_the_resident_grid(aon):
    """2^20 small units: 256 tiles of 4096 distinct units that share their packed bytes, each unit
    with a slot and canaries of its own (about 300 MB of output). Every 64 consecutive list
    entries hold one unit that expands to 4 .. 8 KiB (or overruns an 8-KiB slot) among 63 units
    of 0 .. 12 packed bytes and small slots, a quarter to a third of them failing with
    UNEXPECTED_EOF, OUT_OF_SPACE or INVALID_ARGUMENT (small_streams.refill).
    launch_decode starts min(ceil(n / 256), resident) blocks of decode_small_kernel; on the
    MI355X, resident_blocks gives 1024 blocks (4 per CU on 256 CUs; read from the launched grid of
    this test in a kernel trace: 262144 work-items in blocks of 256), 262144 lanes. 2^20 units are
    4 times that: each wave owns 256 list entries, so every lane takes about 4 units as its earlier
    ones end, at different times, and each wave refills its 64-entry cache three times. (The group
    kernel's grid in the same trace is 768 blocks of 4 waves: 342 entries a wave, group after
    group.) Compared in numpy against the 4096 reference
    results: status and out_len of every unit, and every byte of the output buffer -- decoded
    bytes, canaries, and the slots of failed units where they must stay untouched."""
    r = ss.refill()
    t = r.tile
    tiles = r.n // ss.REFILL_TILE
    assert r.n >= 2 * 1024 * 256
    j = r.order % ss.REFILL_TILE
    d_in = torch.from_numpy(ss.packed_stream(t.units, t.in_off, t.in_end)).to(DEV)
    in_len = np.array([len(u) for u in t.units], dtype=np.int64)[j]
    with all_or_nothing(aon):
        out, ol, st, sz_len, sz_st = run_arrays(d_in, r.in_off, in_len, tiles * r.stride, r.out_off, r.caps)
    verdict = [ss.outcome(e, c, len(u), m) for u, e, c, m in zip(t.units, t.exp, t.caps, t.mis)]
    want_st = np.array([v[0] for v in verdict], dtype=np.int32)[j]
    want_len = np.array([v[1] for v in verdict], dtype=np.int64)[j]
    bad = np.flatnonzero(st != want_st)
    assert bad.size == 0, ("status", bad.size, int(bad[0]), t.kinds[j[bad[0]]], int(st[bad[0]]), int(want_st[bad[0]]))
    bad = np.flatnonzero(ol != want_len)
    assert bad.size == 0, ("out_len", bad.size, int(bad[0]), t.kinds[j[bad[0]]], int(ol[bad[0]]), int(want_len[bad[0]]))
    want_sz_st = np.array([e.size_st for e in t.exp], dtype=np.int32)[j]
    want_sz = np.array([e.size if e.size_st == oracle.OK else 0 for e in t.exp], dtype=np.int64)[j]
    assert np.array_equal(sz_st, want_sz_st) and np.array_equal(sz_len, want_sz)
    care = r.care_strict if aon else r.care_prefix
    out = out.reshape(tiles, r.stride)
    starts = np.sort(t.out_off)
    for t0 in range(0, tiles, 16):
        wrong = (out[t0:t0 + 16] != r.image) & care
        if wrong.any():
            tt, at = (int(x[0]) for x in np.nonzero(wrong))
            unit = int(np.argsort(t.out_off)[max(np.searchsorted(starts, at + ss.FRONT, side="right") - 1, 0)])
            raise AssertionError(("byte", t0 + tt, at, "near unit", unit, t.kinds[unit], len(t.units[unit]),
                                  t.caps[unit], int(t.out_off[unit]), int(wrong.sum())))


# ---- d. class-edge lattice ------------------------------------------------------------------

def lattice_case(aon, decoder):
    b, _ = ss.lattice()
    seen = decode_and_check(b, aon, decoder)
    assert seen == {oracle.OK, oracle.OUT_OF_SPACE}


@both_small_decoders
def test_class_edge_lattice(decoder, aon):
    """Valid streams of exactly 511, 512, 513 packed bytes, of every mid bin edge and the byte after
    it, and of the last length of 320 pieces and the first of 321, at all 16 alignments, in slots
    of the exact size, 8 short, 1 over, 1 short, 8184, 8192 and 8200 B; 00 FF x 4 into 8192 B and
    00 FF x 4, 00 00 into 8200 B. Whichever class a unit lands in, its result is the oracle's."""
    lattice_case(aon, decoder)


@both_small_decoders
def test_class_edge_lattice_auto(aon):
    with cp.decoder("auto"):
        lattice_case(aon, "auto")


# ---- e. the group kernel's cuts -------------------------------------------------------------

def test_group_kernel_cuts():
    """decode_small_group_kernel on hand-built runs of consecutive small units
    (small_streams.group_batches; the grouping each run provokes is computed from the kernel's
    rule in tests/test_small_streams.py): a cut by the piece sum (eight units of 33 pieces), a
    capacity-word sum of exactly 1024 and one of 1025, a lone 8-KiB slot, cap-0 units, empty units
    and a misaligned slot inside a group, a failing unit first, in the middle and last in a group."""
    batches, _ = ss.group_batches()
    seen = set()
    for b in batches:
        seen |= decode_and_check(b, True)
    assert seen == {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE, oracle.INVALID_ARGUMENT}
