"""The default batch encoders (capnp_packed_encode_batch / capnp_packed_encoded_size_batch under
the Zig rule: encode_stream_kernel for small units, encode_kernel for mid units,
long_tiles_kernel + tile_encode_kernel for long ones, behind class_scatter_kernel<4>; DESIGN.md
§2.6) on adversarial and class-edge input, unit by unit and byte for byte against the oracle's
packPacked (message.zig:200-271). The inputs are tests/encode_streams.py's, judged on the CPU by
tests/test_encode_streams.py:
- the small lattice: 0 .. 66 words of a dozen A/B/C/Z patterns at both input phases and every
  slot `address & 15` (a tag, a literal word and a count byte at every position of a 16-B output
  chunk; count bytes patched in registers and after the chunk's store), and waves that alternate
  all-A and all-Z units;
- runs of 255 .. 513 Z or A words with every breaker, their start and end on every lane
  boundary and around 64, 256, 504 and 512 words;
- long units of 2 to 4 tiles with runs against the tile bounds (second and third lookback
  pass, first break 255 / 256 / 257 words past a tile end, units that end on a tile end);
- every class-edge length at both phases and five zero densities, with the in-contract error
  units;
- capacity walks: small units at every capacity 0 .. need + 1, mid and long units around their
  need and the tile ends;
- small units as a minority among mid and long ones, small-only batches around the wave, block
  and class-block sizes, and class blocks without some length bins, also under the launch flags
  and with a caller's workspace.
Every slot lies between 64 sentinel bytes; every test runs encoded_size_batch on the same units
(for long units the tile write pass's totals-only branch) and holds both calls to
encode_streams.check: status, out_len, bytes, [out_len, cap) of an OK unit still sentinel,
nothing outside a slot written, an error unit's slot untouched."""
import numpy as np
import pytest

import capnp_packed as cp
import encode_streams as es

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda"


def i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV)


def run(b, ws=None):
    """encode_batch into a buffer of SENT, and encoded_size_batch, of the same units. Returns the
    host results and the device tensors (output, out_len) for a decode from the slots."""
    n = len(b.units)
    d_in = torch.from_numpy(es.input_buffer(b)).to(DEV)
    in_off, in_len = i64(b.in_off), i64([len(u) for u in b.units])
    d_out = torch.full((es.output_bytes(b),), es.SENT, dtype=torch.uint8, device=DEV)
    out_len = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    status = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    sz_len = torch.full((n,), -1, dtype=torch.int64, device=DEV)
    sz_st = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    cp.encode_batch(d_in, in_off, in_len, d_out, i64(b.out_off), i64(b.caps), out_len, status, ws=ws)
    cp.encoded_size_batch(d_in, in_off, in_len, sz_len, sz_st)
    torch.cuda.synchronize()
    host = (d_out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy(), sz_len.cpu().numpy(),
            sz_st.cpu().numpy())
    return host, (d_out, out_len)


def encode_and_check(b, ws=None):
    (out, ol, st, sz_len, sz_st), dev = run(b, ws)
    seen = es.check(b, out, ol, st)
    es.check(b, None, sz_len, sz_st)
    return seen, (ol, st), dev


@pytest.mark.parametrize("name", ["small_lattice", "run_edges", "tile_edges", "cap_cuts"])
def test_builder(name):
    b = es.BUILDERS[name]()
    seen, _, _ = encode_and_check(b)
    assert seen == es.STATUSES[name]


def test_class_edges(decoder):
    """The class-edge units against the oracle; then their OK outputs, still in their slots, are
    decoded by decode_batch under each mid-unit decoder and must give the inputs back. The empty
    unit at a misaligned start is INVALID_ARGUMENT (include/capnp_packed.h)."""
    b = es.class_edges()
    seen, (ol, st), (d_out, _) = encode_and_check(b)
    assert seen == es.STATUSES["class_edges"]
    i = b.kinds.index("empty at 5 mod 8")
    assert (int(st[i]), int(ol[i])) == (cp.INVALID_ARGUMENT, 0)
    ok = np.flatnonzero(st == cp.OK)
    assert ok.size == len(es.CLASS_LENGTHS) * 2 * len(es.DENSITIES)
    lens = np.array([len(b.units[j]) for j in ok], dtype=np.int64)
    back_off = np.concatenate(([0], np.cumsum(lens + 64)[:-1])) + 64
    back = torch.full((int(back_off[-1] + lens[-1]) + 64,), es.SENT, dtype=torch.uint8, device=DEV)
    dlen = torch.full((ok.size,), -1, dtype=torch.int64, device=DEV)
    dst = torch.full((ok.size,), -1, dtype=torch.int32, device=DEV)
    cp.decode_batch(d_out, i64(b.out_off[ok]), i64(ol[ok]), back, i64(back_off), i64(lens), dlen, dst)
    torch.cuda.synchronize()
    back, dlen, dst = back.cpu().numpy(), dlen.cpu().numpy(), dst.cpu().numpy()
    assert (dst == cp.OK).all() and (dlen == lens).all()
    image = np.full(back.size, es.SENT, dtype=np.uint8)
    for j, o in zip(ok, back_off):
        image[o:o + len(b.units[j])] = np.frombuffer(b.units[j], dtype=np.uint8)
    assert np.array_equal(back, image)


@pytest.mark.parametrize("key", es.MIXED, ids=str)
def test_mixed_batches(key):
    b = es.mixed_batch(key)
    seen, _, _ = encode_and_check(b)
    assert seen == es.statuses(b) <= es.STATUSES["mixed"]


@pytest.mark.parametrize("flags", [cp.LAUNCH_CLASS_SCAN, cp.LAUNCH_MID_SIDE_STREAM | cp.LAUNCH_LONG_INLINE],
                         ids=["class_scan", "mid_side_long_inline"])
@pytest.mark.parametrize("key", ["minority", "blocks3"])
def test_mixed_batches_under_launch_flags(key, flags):
    """The scanned form of the small list's (class block, length bin) order, and the other launch
    orders of the three classes' kernels: no result depends on them."""
    b = es.mixed_batch(key)
    with cp.launch_flags(flags):
        seen, _, _ = encode_and_check(b)
    assert seen == es.statuses(b)


@pytest.mark.parametrize("key", ["minority", "blocks3"])
def test_mixed_batches_with_a_workspace(key):
    b = es.mixed_batch(key)
    seen, _, _ = encode_and_check(b, ws=cp.workspace(len(b.units)))
    assert seen == es.statuses(b)
