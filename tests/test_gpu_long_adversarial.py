"""The long-unit decoders on adversarial and window-edge input, unit by unit and
bit for bit against the oracle's unpackPacked / estimateUnpackedSize (message.zig:88-191): the
window-parallel form (long_windows_kernel, window_spec_kernel, window_resolve_kernel,
window_fill_kernel) and the serial form (decode_wave_kernel<kWvLong>), both on the machinery of
csrc/kernels/decode_wave.h. The inputs are tests/long_streams.py's, judged on the CPU by
tests/test_long_streams.py: random bytes, random bytes closed at a record boundary, one replaced
tag or count, cut tails in the first and last window and at the resolve pass's batch edge, streams
whose chains never meet, a record ending at every depth 0 .. 72 past X_1, X_2, X_31, X_32 and
X_33, unit lengths around the window size, runs across the expand pass's 1024-word lists, and
the mid / long class edge at every alignment. Every unit of every batch is checked: status,
out_len, decoded bytes, and the sentinel in [out_len, cap), in both guard zones, in every gap and
in the whole slot of a failed long unit.
- a batch per family, and decoded_size_batch on the same units (the size pass's own use of the
  spec and resolve kernels);
- every family in one batch among small and mid encoder output, on the library's queue, on a
  caller workspace and with the long units launched inline;
- the serial decoder: about 1 MB of distinct units listed until the batch's windows exceed the
  window table, every alias checked on the device."""
import numpy as np
import pytest

import capnp_packed as cp
import oracle
import long_streams as ls

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"


def dev64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def results(n):
    return torch.full((n,), -1, dtype=torch.int64, device=DEV), torch.full((n,), -1, dtype=torch.int32, device=DEV)


def decode_and_check(b, ws=None, sizes=True):
    """decode_batch of batch b into a buffer of SENT held to ls.check, then decoded_size_batch of
    the same units held to oracle.decoded_size. Returns the statuses met, counted."""
    n = len(b.units)
    d_in = torch.from_numpy(ls.packed_stream(b)).to(DEV)
    d_off, d_len = dev64(b.in_off), dev64([len(u) for u in b.units])
    d_out = torch.full((b.out_end,), ls.SENT, dtype=torch.uint8, device=DEV)
    out_len, status = results(n)
    cp.decode_batch(d_in, d_off, d_len, d_out, dev64(b.out_off), dev64(b.caps), out_len, status, ws=ws)
    torch.cuda.synchronize()
    seen = ls.check(b, status.cpu().numpy(), out_len.cpu().numpy(), d_out.cpu().numpy())
    if sizes:
        sz_len, sz_st = results(n)
        cp.decoded_size_batch(d_in, d_off, d_len, sz_len, sz_st)
        torch.cuda.synchronize()
        ls.check_sizes(b, sz_len.cpu().numpy(), sz_st.cpu().numpy())
    return seen


@pytest.mark.parametrize("name", ls.FAMILIES)
def test_family(name):
    b = ls.family_batch(name)
    seen = decode_and_check(b)
    want = {ls.outcome(e, c, m)[0] for e, c, m in zip(b.exp, b.caps, b.mis)}
    assert set(seen) == want and sum(seen.values()) == len(b.units)


@pytest.mark.parametrize("how", ["queue", "workspace", "long_inline"])
def test_all_families_one_batch(how):
    """Every family's units shuffled among 300 small and mid units of encoder output: the long and
    huge units share the class pass and the side stream with the other classes."""
    b = ls.all_families()
    if how == "long_inline":
        prev = cp.set_launch_flags(cp.LAUNCH_LONG_INLINE)
        try:
            seen = decode_and_check(b)
        finally:
            cp.set_launch_flags(prev)
    else:
        seen = decode_and_check(b, ws=cp.workspace(len(b.units)) if how == "workspace" else None, sizes=False)
    assert set(seen) == {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE, oracle.INVALID_ARGUMENT}
    assert sum(seen.values()) == len(b.units)


def test_serial_decoder_on_adversarial_units():
    """decode_wave_kernel<kWvLong> (and, for the sizes, the size-only index walk) on closed, phase,
    entry and cut units of 50 KB .. 400 KB: 710 aliases of four device-resident units, equal in_off
    and a slot each, whose windows exceed the window table (n / 8 + 32768), so some of them take
    the serial list; which ones the atomics of long_windows_kernel decide, so every alias is
    compared, on the device."""
    s = ls.serial_batch()
    n = len(s.alias)
    assert s.windows > ls.win_cap(n)
    buf = np.full(s.in_end + 64, 0xFF, dtype=np.uint8)
    for u, o in zip(s.units, s.in_off):
        buf[o:o + len(u)] = np.frombuffer(u, dtype=np.uint8)
    d_in = torch.from_numpy(buf).to(DEV)
    lens = np.array([len(u) for u in s.units], dtype=np.int64)
    d_off, d_len = dev64(s.in_off[s.alias]), dev64(lens[s.alias])
    d_out = torch.full((s.out_end,), ls.SENT, dtype=torch.uint8, device=DEV)
    out_len, status = results(n)
    cp.decode_batch(d_in, d_off, d_len, d_out, dev64(s.out_off), dev64(s.caps), out_len, status)
    torch.cuda.synchronize()
    verdict = [ls.outcome(s.exp[j], int(c)) for j, c in zip(s.alias, s.caps)]
    want_st = np.array([v[0] for v in verdict], dtype=np.int32)
    want_len = np.array([v[1] for v in verdict], dtype=np.int64)
    st, ol = status.cpu().numpy(), out_len.cpu().numpy()
    bad = np.flatnonzero(st != want_st)
    assert bad.size == 0, ("status", bad.size, int(bad[0]), s.kinds[s.alias[bad[0]]], int(st[bad[0]]), int(want_st[bad[0]]))
    bad = np.flatnonzero(ol != want_len)
    assert bad.size == 0, ("out_len", bad.size, int(bad[0]), s.kinds[s.alias[bad[0]]], int(ol[bad[0]]), int(want_len[bad[0]]))
    assert {oracle.OK, oracle.UNEXPECTED_EOF, oracle.OUT_OF_SPACE} == set(want_st.tolist())
    refs = [torch.from_numpy(np.frombuffer(e.ref, dtype=np.uint8).copy()).to(DEV) if e.st == oracle.OK else None
            for e in s.exp]
    written = d_out != ls.SENT  # after the loop: the bytes that differ from the sentinel outside every OK alias's output
    for a in range(n):
        if want_st[a] == oracle.OK:
            o, L = int(s.out_off[a]), int(want_len[a])
            assert torch.equal(d_out[o:o + L], refs[s.alias[a]]), ("decoded bytes", a, s.kinds[s.alias[a]])
            written[o:o + L] = False
    if written.any().item():  # [out_len, cap), the guard zones, the gaps, the failed aliases' slots
        at = int(torch.nonzero(written)[0].item())
        a = int(np.searchsorted(s.out_off - ls.FRONT, at, side="right")) - 1
        raise AssertionError(("sentinel overwritten", at, "alias", a, s.kinds[s.alias[a]], int(want_st[a]),
                              at - int(s.out_off[a]), int(s.caps[a])))
    sz_len, sz_st = results(n)
    cp.decoded_size_batch(d_in, d_off, d_len, sz_len, sz_st)
    torch.cuda.synchronize()
    want_sz_st = np.array([s.exp[j].size_st for j in s.alias], dtype=np.int32)
    want_sz = np.array([s.exp[j].size if s.exp[j].size_st == oracle.OK else 0 for j in s.alias], dtype=np.int64)
    assert np.array_equal(sz_st.cpu().numpy(), want_sz_st) and np.array_equal(sz_len.cpu().numpy(), want_sz)
