"""Host-side mirror of the reference's packed read/write surface over the C-ABI.

The reference (nullstyle/capnp-zig) exposes packing through
  MessageBuilder.toPackedBytes / writePackedTo   src/serialization/message.zig:2175-2213
  Message.initPacked                             message.zig:400-408
  Reader.initPacked                              src/serialization/reader.zig:18-23
over the file-private packPacked / unpackPacked / estimateUnpackedSize
(message.zig:88-271). This module keeps those names, argument meanings and error
names, and routes every byte through libcapnp_packed.so (HIP kernels for gfx950).
There is no CPU fallback: if the library or a gfx950 device is missing, calls
raise NoDevice / RuntimeError.

Batch functions take torch tensors that live in device memory (torch is used only
for device memory and streams): uint8 byte buffers, int64 offset/length tensors
(bit-identical to the ABI's u64), int32 status tensors.
"""
from __future__ import annotations

import ctypes
from collections import deque
import gc
import os
import struct

import numpy as np

try:  # load torch first so libcapnp_packed.so binds to the same HIP runtime instance
    import torch
except ImportError:  # pragma: no cover - the ABI still loads for symbol checks
    torch = None

HERE = os.path.dirname(os.path.abspath(__file__))
# CPK_LIB selects an experimental build of the same library (scripts/ diagnostics only)
LIB_PATH = os.environ.get("CPK_LIB") or os.path.join(HERE, "lib", "libcapnp_packed.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "capnp_packed.h")

OK = 0
INVALID_MESSAGE_SIZE = 1
UNEXPECTED_EOF = 2
OVERFLOW = 3
OUT_OF_SPACE = 4
INVALID_ARGUMENT = 5
DEVICE_ERROR = 6
NO_DEVICE = 7
# Reader.readPackedMessage (reader.zig:84-156)
END_OF_STREAM = 8
INVALID_SEGMENT_COUNT = 9
SEGMENT_COUNT_LIMIT_EXCEEDED = 10
MESSAGE_TOO_LARGE = 11
INVALID_PACKED_MESSAGE = 12
# Message.init (message.zig:341-394)
TRUNCATED_MESSAGE = 13
# Message.validate (message.zig:699-969)
EMPTY_MESSAGE = 14
NESTING_LIMIT_EXCEEDED = 15
INVALID_SEGMENT_ID = 16
INVALID_POINTER = 17
OUT_OF_BOUNDS = 18
TRAVERSAL_LIMIT_EXCEEDED = 19
INVALID_FAR_POINTER = 20
INVALID_INLINE_COMPOSITE_POINTER = 21
LIST_TOO_LARGE = 22


class PackedError(Exception):
    status = -1


class InvalidMessageSize(PackedError):  # message.zig:201
    status = INVALID_MESSAGE_SIZE


class UnexpectedEof(PackedError):  # message.zig:152-191
    status = UNEXPECTED_EOF


class Overflow(PackedError):  # message.zig:163
    status = OVERFLOW


class OutOfSpace(PackedError):
    status = OUT_OF_SPACE


class InvalidArgument(PackedError):
    status = INVALID_ARGUMENT


class DeviceError(PackedError):
    status = DEVICE_ERROR


class NoDevice(PackedError):
    status = NO_DEVICE


# Message.init (message.zig:341-394) and Reader.readPackedMessage (reader.zig:84-156) errors
class EndOfStream(PackedError):
    status = END_OF_STREAM


class InvalidSegmentCount(PackedError):
    status = INVALID_SEGMENT_COUNT


class SegmentCountLimitExceeded(PackedError):
    status = SEGMENT_COUNT_LIMIT_EXCEEDED


class MessageTooLarge(PackedError):  # reader.zig:140
    status = MESSAGE_TOO_LARGE


class InvalidPackedMessage(PackedError):  # reader.zig:151-153
    status = INVALID_PACKED_MESSAGE


class TruncatedMessage(PackedError):  # message.zig:353/380
    status = TRUNCATED_MESSAGE


# Message.validate (message.zig:699-969)
class EmptyMessage(PackedError):  # :700
    status = EMPTY_MESSAGE


class NestingLimitExceeded(PackedError):  # :717
    status = NESTING_LIMIT_EXCEEDED


class InvalidSegmentId(PackedError):  # :718 / :421 / :739
    status = INVALID_SEGMENT_ID


class InvalidPointer(PackedError):  # :731
    status = INVALID_POINTER


class OutOfBounds(PackedError):  # bounds.zig:10-13
    status = OUT_OF_BOUNDS


class TraversalLimitExceeded(PackedError):  # :711
    status = TRAVERSAL_LIMIT_EXCEEDED


class InvalidFarPointer(PackedError):  # :752-758
    status = INVALID_FAR_POINTER


class InvalidInlineCompositePointer(PackedError):  # :600-612 / :944
    status = INVALID_INLINE_COMPOSITE_POINTER


class ListTooLarge(PackedError):  # :949
    status = LIST_TOO_LARGE


_ERRORS = {c.status: c for c in (InvalidMessageSize, UnexpectedEof, Overflow, OutOfSpace,
                                 InvalidArgument, DeviceError, NoDevice, EndOfStream, InvalidSegmentCount,
                                 SegmentCountLimitExceeded, MessageTooLarge, InvalidPackedMessage,
                                 TruncatedMessage, EmptyMessage, NestingLimitExceeded, InvalidSegmentId,
                                 InvalidPointer, OutOfBounds, TraversalLimitExceeded, InvalidFarPointer,
                                 InvalidInlineCompositePointer, ListTooLarge)}


_lib = None
_vp = ctypes.c_void_p
_sz = ctypes.c_size_t

# exported symbol -> (restype, argtypes)
SIGNATURES = {
    "capnp_packed_abi_version": (ctypes.c_uint32, []),
    "capnp_packed_last_error": (ctypes.c_char_p, []),
    "capnp_packed_status_name": (ctypes.c_char_p, [ctypes.c_int]),
    "capnp_packed_encode_bound": (_sz, [_sz]),
    "capnp_packed_encode": (ctypes.c_int, [_vp, _sz, _vp, _sz, ctypes.POINTER(_sz)]),
    "capnp_packed_encode_dialect": (ctypes.c_int, [_vp, _sz, _vp, _sz, ctypes.POINTER(_sz), ctypes.c_uint32]),
    "capnp_packed_encode_batch_dialect": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                                         ctypes.c_uint32, _vp, _sz, _vp]),
    "capnp_packed_encode_message_batch_dialect": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp,
                                                                 _vp, _vp, ctypes.c_uint32, _vp]),
    "capnp_packed_encode_dense_workspace_bytes": (_sz, [ctypes.c_uint32]),
    "capnp_packed_encode_dense_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64,
                                                       ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, _vp, _sz,
                                                       _vp]),
    "capnp_packed_encode_framed": (ctypes.c_int, [_vp, _sz, _vp, _sz, ctypes.POINTER(_sz), ctypes.c_uint32]),
    "capnp_packed_encode_framed_workspace_bytes": (_sz, [ctypes.c_uint32]),
    "capnp_packed_encode_framed_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                                        ctypes.c_uint32, _vp, _sz, _vp]),
    "capnp_packed_encode_framed_dense_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint64,
                                                              ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, _vp,
                                                              _sz, _vp]),
    "capnp_packed_split_workspace_bytes": (_sz, [ctypes.c_uint32, ctypes.c_uint64]),
    "capnp_packed_split_streams": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint64, _vp, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "capnp_packed_decoded_size": (ctypes.c_int, [_vp, _sz, ctypes.POINTER(_sz)]),
    "capnp_packed_decode": (ctypes.c_int, [_vp, _sz, _vp, _sz, ctypes.POINTER(_sz)]),
    "capnp_packed_encode_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "capnp_packed_encoded_size_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    "capnp_packed_decode_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "capnp_packed_batch_workspace_bytes": (_sz, [ctypes.c_uint32]),
    "capnp_packed_encode_batch_ws": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                                    _sz, _vp]),
    "capnp_packed_decode_batch_ws": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp,
                                                    _sz, _vp]),
    "capnp_packed_decoded_size_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    "capnp_packed_read_message_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp,
                                                       _vp, _vp]),
    "capnp_packed_read_message": (ctypes.c_int, [_vp, _sz, _vp, _sz, ctypes.POINTER(_sz), ctypes.POINTER(_sz)]),
    "capnp_packed_encode_message_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                                         _vp, _vp]),
    "capnp_packed_message_init_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp,
                                                       _vp, _vp, _vp]),
    "capnp_packed_validate_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, ctypes.c_uint64,
                                                   ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp]),
    "capnp_packed_read_fields_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, _vp,
                                                      _vp, _vp, _vp]),
    "capnp_packed_gather_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64, _vp,
                                                 _vp]),
    "capnp_packed_build_fields_batch": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint32, _vp, ctypes.c_uint32,
                                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "capnp_packed_list_heads_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_uint32,
                                                     ctypes.c_uint32, ctypes.c_uint32, _vp, _vp, _vp, _vp]),
    "capnp_packed_read_elements_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32,
                                                        ctypes.c_uint64, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp,
                                                        _vp, _vp, _vp]),
    "capnp_packed_scan_scratch_bytes": (_sz, [ctypes.c_uint32]),
    "capnp_packed_lengths_to_offsets": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint64, _vp, _vp,
                                                       _sz, _vp]),
    "capnp_packed_generate": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                             ctypes.c_uint64, ctypes.c_uint32, _vp]),
    "capnp_packed_frame_connections": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, _vp, ctypes.c_uint32, _vp, _vp,
                                                      ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp,
                                                      ctypes.POINTER(ctypes.c_uint32)]),
    "capnp_packed_stream_release": (ctypes.c_int, [_vp]),
    "capnp_packed_stream_contexts": (ctypes.c_int, [ctypes.POINTER(ctypes.c_uint32)]),
    "capnp_packed_stream_queue_info": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_size_t),
                                                      ctypes.POINTER(ctypes.c_uint32)]),
    "capnp_packed_set_decoder": (ctypes.c_int, [ctypes.c_int]),
    "capnp_packed_set_all_or_nothing": (ctypes.c_int, [ctypes.c_int]),
    "capnp_packed_set_launch_flags": (ctypes.c_uint32, [ctypes.c_uint32]),
    "capnp_packed_framer_create": (ctypes.c_int, [ctypes.c_uint32, ctypes.POINTER(_vp)]),
    "capnp_packed_framer_destroy": (ctypes.c_int, [_vp]),
    "capnp_packed_framer_read": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp,
                                                _vp, ctypes.c_uint32, _vp, ctypes.POINTER(ctypes.c_uint32)]),
    "capnp_packed_framer_readv": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp, _vp,
                                                 ctypes.c_uint32, _vp, ctypes.POINTER(ctypes.c_uint32)]),
    "capnp_packed_framer_reset": (ctypes.c_int, [_vp, ctypes.c_uint32]),
    "capnp_packed_framer_buffered": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]),
    "capnp_packed_framer_expected": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]),
    "capnp_packed_framer_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64),
                                                 ctypes.POINTER(ctypes.c_uint64)]),
    "capnp_packed_framer_walk_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint64),
                                                      ctypes.POINTER(ctypes.c_uint64)]),
}

# capnp_packed_set_decoder values (include/capnp_packed.h)
DECODERS = {"auto": 0, "twopass": 1, "fused": 2, "stream": 3, "words": 4}
# encoder dialects (include/capnp_packed.h): "zig" = packPacked's bytes (the default everywhere),
# "cxx" = the bytes of the C++ capnp packer and pycapnp (opt-in)
DIALECTS = {"zig": 0, "cxx": 1}
# capnp_packed_set_launch_flags bits (include/capnp_packed.h)
LAUNCH_LONG_INLINE = 0x1
LAUNCH_MID_SIDE_STREAM = 0x2
LAUNCH_CLASS_SCAN = 0x4


def lib():
    """Load libcapnp_packed.so (built by `make -C capnp-zig_amd`). Fails loudly."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C capnp-zig_amd` "
                               "(there is no CPU fallback)")
        L = ctypes.CDLL(LIB_PATH)
        dev_build = "CPK_LIB" in os.environ  # an older dev build (same-box A/B) may lack newer entry points
        for name, (res, args) in SIGNATURES.items():
            if dev_build and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return lib().capnp_packed_last_error().decode()


def _raise(st: int, what: str = ""):
    if st == OK:
        return
    cls = _ERRORS.get(st, PackedError)
    raise cls(f"{what}: {lib().capnp_packed_status_name(st).decode()} ({last_error()})")


def _dialect(dialect) -> int:
    try:
        return DIALECTS[dialect]
    except (KeyError, TypeError):
        raise InvalidArgument(f"dialect must be 'zig' or 'cxx', not {dialect!r}") from None


def _cbuf(data) -> ctypes.Array:
    b = bytes(data)
    return ctypes.create_string_buffer(b, max(1, len(b)))


# ---------------------------------------------------------------------------
# single-buffer API (host bytes in, host bytes out; one unit through the GPU)
# ---------------------------------------------------------------------------

def encode_bound(n: int) -> int:
    return lib().capnp_packed_encode_bound(n)


def pack_packed(data, dialect="zig") -> bytes:
    """packPacked (message.zig:200-271). Raises InvalidMessageSize if len % 8.
    dialect="cxx": the C++ capnp packer's bytes of the buffer as one piece."""
    d = _dialect(dialect)
    data = bytes(data)
    cap = encode_bound(len(data))
    out = ctypes.create_string_buffer(max(1, cap))
    n = _sz()
    if d == 0:
        st = lib().capnp_packed_encode(_cbuf(data), len(data), out, cap, ctypes.byref(n))
    else:
        st = lib().capnp_packed_encode_dialect(_cbuf(data), len(data), out, cap, ctypes.byref(n), d)
    _raise(st, "packPacked")
    return out.raw[:n.value]


def pack_message(framed, dialect="zig") -> bytes:
    """One framed message (toBytes' bytes) packed (capnp_packed_encode_framed). dialect="cxx":
    the segment table and each segment as pieces of their own, the bytes of capnp convert
    binary:packed and pycapnp; "zig": packPacked(framed). The message must be exactly its table
    plus its segments (TruncatedMessage and the table errors; InvalidArgument for trailing words)."""
    d = _dialect(dialect)
    framed = bytes(framed)
    cap = encode_bound(len(framed) - len(framed) % 8)
    out = ctypes.create_string_buffer(max(1, cap))
    n = _sz()
    st = lib().capnp_packed_encode_framed(_cbuf(framed), len(framed), out, cap, ctypes.byref(n), d)
    _raise(st, "packMessage")
    return out.raw[:n.value]


def estimate_unpacked_size(packed) -> int:
    """estimateUnpackedSize (message.zig:152-191)."""
    packed = bytes(packed)
    n = _sz()
    st = lib().capnp_packed_decoded_size(_cbuf(packed), len(packed), ctypes.byref(n))
    _raise(st, "estimateUnpackedSize")
    return n.value


def unpack_packed(packed, size_hint=None) -> bytes:
    """unpackPacked (message.zig:88-145). Raises UnexpectedEof on truncation.
    One device decode into a buffer of `size_hint` bytes (default 4 x the packed length):
    a message that needs more ends OUT_OF_SPACE with its size, and is decoded again into
    a buffer of exactly that size (the reference sizes first, message.zig:90)."""
    packed = bytes(packed)
    cap = max(4096, 4 * len(packed)) if size_hint is None else int(size_hint)
    for _ in range(2):
        out = ctypes.create_string_buffer(max(1, cap))
        n = _sz()
        st = lib().capnp_packed_decode(_cbuf(packed), len(packed), out, cap, ctypes.byref(n))
        if st == OUT_OF_SPACE and n.value > cap:
            cap = n.value
            continue
        _raise(st, "unpackPacked")
        return out.raw[:n.value]
    _raise(st, "unpackPacked")


# ---------------------------------------------------------------------------
# framing mirror: MessageBuilder / Message / Reader (packed entry points only)
# ---------------------------------------------------------------------------

MAX_SEGMENT_COUNT = 512  # message.zig:310


def frame_segments(segments) -> bytes:
    """MessageBuilder.toBytes (message.zig:2123-2170): segment table + segments."""
    segs = [bytes(s) for s in segments] or [b""]
    n = len(segs)
    for s in segs:
        if len(s) % 8:
            raise InvalidMessageSize("segment length is not a multiple of 8")
    hdr = struct.pack("<I", n - 1) + b"".join(struct.pack("<I", len(s) // 8) for s in segs)
    if n % 2 == 0:
        hdr += b"\x00\x00\x00\x00"
    return hdr + b"".join(segs)


class MessageBuilder:
    """Mirror of MessageBuilder (message.zig:1643): the serialization surface over segments the
    caller gives, and single-segment struct building (allocate_struct), which records builder
    calls and runs them as one n = 1 capnp_packed_build_fields_batch call on the device in
    to_bytes(); there is no CPU path. The two do not mix: allocate_struct wants an empty message
    and create_segment refuses once a root is recorded. Struct lists, pointer lists and other
    segments are out of scope."""

    def __init__(self, device="cuda"):
        self.segments: list[bytearray] = []
        self.device = device
        self._ops: list = []     # BuildOp, in call order
        self._values: list = []  # per op: an int (data kinds), bytes (slices) or None (structs)
        self._counts: list = []

    def create_segment(self, data=b"") -> int:
        if self._ops:
            raise InvalidArgument("a message built by allocate_struct has segment 0 only")
        self.segments.append(bytearray(data))
        return len(self.segments) - 1

    def allocate_struct(self, data_words: int, pointer_words: int) -> "StructBuilder":
        """allocateStruct (message.zig:2061-2101) of the root struct in segment 0."""
        if self._ops or self.segments:
            raise InvalidArgument("allocate_struct builds the root of an empty message")
        return StructBuilder(self, self._record(BuildOp(BUILD_STRUCT, 0, data_words=data_words,
                                                        pointer_words=pointer_words), None))

    def _record(self, op, value, count=0) -> int:
        self._ops.append(op)
        self._values.append(value)
        self._counts.append(count)
        return len(self._ops) - 1

    def _build(self) -> bytes:
        nops = len(self._ops)
        pool = bytearray()
        cols = np.zeros((3, nops), dtype=np.uint64)
        for k, v in enumerate(self._values):
            if isinstance(v, (bytes, bytearray)):
                cols[0, k], cols[1, k], cols[2, k] = len(pool), len(v), self._counts[k]
                pool += v
            elif v is not None:
                cols[0, k] = v
        dev = self.device
        d_pool = torch.from_numpy(np.frombuffer(bytes(pool) + b"\0" * 16, dtype=np.uint8).copy()).to(dev)
        d_cols = torch.from_numpy(cols.view(np.int64)).to(dev)
        out_len = torch.zeros(1, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        build_fields_batch(d_pool, self._ops, d_cols[0], d_cols[1], None, None, None, out_len, status, d_cols[2],
                           pool_len=len(pool))
        _raise(int(status.item()), "MessageBuilder.to_bytes")
        size = int(out_len.item())
        d_out = torch.empty(size, dtype=torch.uint8, device=dev)
        off = torch.zeros(1, dtype=torch.int64, device=dev)
        build_fields_batch(d_pool, self._ops, d_cols[0], d_cols[1], d_out, off, out_len.clone(), out_len, status,
                           d_cols[2], pool_len=len(pool))
        _raise(int(status.item()), "MessageBuilder.to_bytes")
        return d_out.cpu().numpy().tobytes()

    def to_bytes(self) -> bytes:
        if self._ops:
            framed = self._build()
            self.segments = [bytearray(framed[8:])]  # one segment: an 8-byte table
            return framed
        if not self.segments:
            self.create_segment()
        return frame_segments(self.segments)

    def to_packed_bytes(self, dialect="zig") -> bytes:
        """message.zig:2175-2179: packPacked(toBytes()). dialect="cxx": the bytes the C++
        message writer gives these segments (table and segments packed piece by piece)."""
        if _dialect(dialect) == 0:
            return pack_packed(self.to_bytes())
        if not self.segments:
            self.create_segment()
        return pack_message_cxx(self.segments)

    def write_to(self, writer) -> None:
        writer.write(self.to_bytes())

    def write_packed_to(self, writer, dialect="zig") -> None:
        """message.zig:2209-2213."""
        writer.write(self.to_packed_bytes(dialect))


class StructBuilder:
    """Mirror of StructBuilder (message/struct_builder.zig:332-989) for one struct of a
    MessageBuilder's segment 0: every write records one op of the message's build."""

    def __init__(self, message: MessageBuilder, op_index: int):
        self.message, self.op_index = message, op_index

    def _data(self, kind, byte_offset, value, bit=0):
        self.message._record(BuildOp(kind, byte_offset, bit, self.op_index), int(value))

    def _slice(self, kind, pointer_index, data, count=0):
        self.message._record(BuildOp(kind, pointer_index, 0, self.op_index), bytes(data), count)

    def write_u8(self, byte_offset: int, value: int) -> None:
        self._data(FIELD_U8, byte_offset, value & 0xFF)

    def write_u16(self, byte_offset: int, value: int) -> None:
        self._data(FIELD_U16, byte_offset, value & 0xFFFF)

    def write_u32(self, byte_offset: int, value: int) -> None:
        self._data(FIELD_U32, byte_offset, value & 0xFFFFFFFF)

    def write_u64(self, byte_offset: int, value: int) -> None:
        self._data(FIELD_U64, byte_offset, value & 0xFFFFFFFFFFFFFFFF)

    def write_bool(self, byte_offset: int, bit_offset: int, value: bool) -> None:
        self._data(FIELD_BOOL, byte_offset, 1 if value else 0, bit_offset)

    def write_text(self, pointer_index: int, text) -> None:
        self._slice(FIELD_TEXT, pointer_index, text.encode() if isinstance(text, str) else text)

    def write_data(self, pointer_index: int, data) -> None:
        self._slice(FIELD_DATA, pointer_index, data)

    def write_u16_list(self, pointer_index: int, values) -> None:
        self._slice(FIELD_LIST_16, pointer_index, np.asarray(values, dtype="<u2").tobytes())

    def write_u32_list(self, pointer_index: int, values) -> None:
        self._slice(FIELD_LIST_32, pointer_index, np.asarray(values, dtype="<u4").tobytes())

    def write_u64_list(self, pointer_index: int, values) -> None:
        self._slice(FIELD_LIST_64, pointer_index, np.asarray(values, dtype="<u8").tobytes())

    def write_bool_list(self, pointer_index: int, values) -> None:
        bits = np.asarray(values, dtype=bool)
        self._slice(FIELD_LIST_BIT, pointer_index, np.packbits(bits, bitorder="little").tobytes(), len(bits))

    def init_struct(self, pointer_index: int, data_words: int, pointer_words: int) -> "StructBuilder":
        return StructBuilder(self.message, self.message._record(
            BuildOp(BUILD_STRUCT, pointer_index, 0, self.op_index, data_words, pointer_words), None))


class Message:
    """Mirror of Message (message.zig:309-418): segment views over backing data."""

    def __init__(self, segments, backing_data):
        self.segments = segments
        self.backing_data = backing_data

    @classmethod
    def init(cls, data) -> "Message":
        """message.zig:341-394 segment-table parse; borrows `data`."""
        mv = memoryview(bytes(data) if not isinstance(data, (bytes, bytearray, memoryview)) else data)
        if len(mv) < 4:
            raise EndOfStream()
        (minus_one,) = struct.unpack_from("<I", mv, 0)
        if minus_one == 0xFFFFFFFF:
            raise InvalidSegmentCount()
        count = minus_one + 1
        if count > MAX_SEGMENT_COUNT:
            raise SegmentCountLimitExceeded()
        header_bytes = (1 + count + (1 if count % 2 == 0 else 0)) * 4
        if header_bytes > len(mv):
            raise TruncatedMessage()
        sizes = struct.unpack_from(f"<{count}I", mv, 4)
        off = header_bytes
        segs = []
        for sw in sizes:
            end = off + 8 * sw
            if end > len(mv):
                raise TruncatedMessage()
            segs.append(mv[off:end])
            off = end
        return cls(segs, None)

    @classmethod
    def init_packed(cls, packed) -> "Message":
        """message.zig:400-408: unpackPacked then Message.init; owns the buffer."""
        unpacked = unpack_packed(packed)
        msg = cls.init(unpacked)
        msg.backing_data = unpacked
        return msg

    def validate(self, segment_count_limit=None, traversal_limit_words=None, nesting_limit=None,
                 device="cuda") -> int:
        """message.zig:699-969 Message.validate(options), run by validate_batch on the
        device over this message's segments (re-framed: header + segments, the bytes
        Message.init parsed). Raises the reference's error; returns the traversal words
        consumed. Arguments left None take ValidationOptions' defaults (:331-335).
        An empty segment list raises EmptyMessage (:700), as after deinit(). Segments are
        whole words when they come from Message.init / init_packed; a hand-built segment
        whose length is not a multiple of 8 cannot be framed and raises InvalidMessageSize."""
        if len(self.segments) == 0:
            raise EmptyMessage("Message.validate: no segments")
        framed = np.frombuffer(frame_segments(self.segments), dtype=np.uint8)
        d_in = torch.from_numpy(framed.copy()).to(device)
        off = torch.zeros(1, dtype=torch.int64, device=device)
        ln = torch.full((1,), framed.size, dtype=torch.int64, device=device)
        st = torch.full((1,), -1, dtype=torch.int32, device=device)
        words = torch.zeros(1, dtype=torch.int64, device=device)
        validate_batch(d_in, off, ln, st, words,
                       DEFAULT_SEGMENT_COUNT_LIMIT if segment_count_limit is None else segment_count_limit,
                       DEFAULT_TRAVERSAL_LIMIT_WORDS if traversal_limit_words is None else traversal_limit_words,
                       DEFAULT_NESTING_LIMIT if nesting_limit is None else nesting_limit)
        _raise(int(st.item()), "Message.validate")
        return int(words.item())

    def get_root_struct(self, device="cuda") -> "StructReader":
        """message.zig:973-985 getRootStruct, resolved on the device (one n = 1
        read_fields_batch call); raises the reference's error."""
        if len(self.segments) == 0:
            raise EmptyMessage("Message.getRootStruct: no segments")
        root = StructReader(self, (), device)
        root._read(FIELD_U8, 0)  # resolves the root: its errors are getRootStruct's
        return root

    def deinit(self) -> None:
        self.segments = []
        self.backing_data = None


class StructReader:
    """Mirror of StructReader (message.zig:1010-1443): the schema-less reads of a struct reached
    from the root by readStruct steps. Every read is one n = 1 capnp_packed_read_fields_batch
    call on the device over the message's framed bytes (slices: plus one gather_batch) and
    raises the reference's error; there is no CPU path."""

    def __init__(self, message: Message, path, device):
        self.message, self.path, self.device = message, tuple(path), device
        self._dev = None

    def _framed(self):
        if self._dev is None:
            framed = np.frombuffer(frame_segments(self.message.segments), dtype=np.uint8)
            self._dev = (torch.from_numpy(framed.copy()).to(self.device),
                         torch.zeros(1, dtype=torch.int64, device=self.device),
                         torch.full((1,), framed.size, dtype=torch.int64, device=self.device))
        return self._dev

    def _read(self, kind, offset, bit=0, what="StructReader"):
        d_in, off, ln = self._framed()
        out = torch.zeros(3, dtype=torch.int64, device=self.device)
        st = torch.full((1,), -1, dtype=torch.int32, device=self.device)
        read_fields_batch(d_in, off, ln, [Field(kind, offset, bit, self.path)], out[0:1], out[1:2], st, out[2:3])
        _raise(int(st.item()), what)
        v, l, c = (int(x) for x in out.cpu().numpy().view(np.uint64))
        return v, l, c

    def _slice(self, kind, index, what) -> tuple:
        v, l, c = self._read(kind, index, what=what)
        d_in = self._framed()[0]
        dst = torch.empty(l, dtype=torch.uint8, device=self.device)
        st = torch.full((1,), -1, dtype=torch.int32, device=self.device)
        gather_batch(d_in, torch.tensor([v], dtype=torch.int64, device=self.device),
                     torch.tensor([l], dtype=torch.int64, device=self.device), dst,
                     torch.zeros(1, dtype=torch.int64, device=self.device), st, cap=l)
        _raise(int(st.item()), what)
        return dst.cpu().numpy().tobytes(), c

    def read_u8(self, byte_offset: int) -> int:
        return self._read(FIELD_U8, byte_offset)[0]

    def read_u16(self, byte_offset: int) -> int:
        return self._read(FIELD_U16, byte_offset)[0]

    def read_u32(self, byte_offset: int) -> int:
        return self._read(FIELD_U32, byte_offset)[0]

    def read_u64(self, byte_offset: int) -> int:
        return self._read(FIELD_U64, byte_offset)[0]

    def read_bool(self, byte_offset: int, bit_offset: int) -> bool:
        return bool(self._read(FIELD_BOOL, byte_offset, bit_offset)[0])

    def read_union_discriminant(self, byte_offset: int) -> int:
        return self.read_u16(byte_offset)

    def read_text(self, pointer_index: int) -> bytes:
        return self._slice(FIELD_TEXT, pointer_index, "StructReader.readText")[0]

    def read_data(self, pointer_index: int) -> bytes:
        return self._slice(FIELD_DATA, pointer_index, "StructReader.readData")[0]

    def _list(self, kind, index, dtype, what) -> list:
        raw, count = self._slice(kind, index, what)
        return np.frombuffer(raw, dtype=dtype)[:count].tolist()

    def read_u16_list(self, pointer_index: int) -> list:
        return self._list(FIELD_LIST_16, pointer_index, "<u2", "StructReader.readU16List")

    def read_u32_list(self, pointer_index: int) -> list:
        return self._list(FIELD_LIST_32, pointer_index, "<u4", "StructReader.readU32List")

    def read_u64_list(self, pointer_index: int) -> list:
        return self._list(FIELD_LIST_64, pointer_index, "<u8", "StructReader.readU64List")

    def read_f32_list(self, pointer_index: int) -> list:
        return self._list(FIELD_LIST_32, pointer_index, "<f4", "StructReader.readF32List")

    def read_f64_list(self, pointer_index: int) -> list:
        return self._list(FIELD_LIST_64, pointer_index, "<f8", "StructReader.readF64List")

    def read_bool_list(self, pointer_index: int) -> list:
        raw, count = self._slice(FIELD_LIST_BIT, pointer_index, "StructReader.readBoolList")
        return [bool((raw[i >> 3] >> (i & 7)) & 1) for i in range(count)]

    def read_struct(self, pointer_index: int) -> "StructReader":
        """readStruct (:1224-1235). The device descriptor holds four steps from the root: a fifth
        raises InvalidArgument."""
        child = StructReader(self.message, self.path + (pointer_index,), self.device)
        child._dev = self._dev
        child._read(FIELD_U8, 0, what="StructReader.readStruct")
        return child


class _ListReader:
    """A list resolved by one n = 1 list_heads_batch call: len(), and element reads that are one
    n = 1 read_elements_batch call each (the element numbering is start = [0, count])."""

    def __init__(self, parent: StructReader, pointer_index: int, kind: int, what: str):
        self.reader, self.kind = parent, kind
        d_in, off, ln = parent._framed()
        dev = parent.device
        self.head = torch.zeros(LIST_HEAD_BYTES, dtype=torch.uint8, device=dev)
        count = torch.zeros(1, dtype=torch.int64, device=dev)
        st = torch.full((1,), -1, dtype=torch.int32, device=dev)
        list_heads_batch(d_in, off, ln, kind, pointer_index, self.head, count, st, parent.path)
        _raise(int(st.item()), what)
        self.count = int(count.item())
        self.host_head = self.head.cpu().numpy().view(LIST_HEAD_DTYPE).copy()

    def len(self) -> int:
        return self.count

    def __len__(self) -> int:
        return self.count

    def _check(self, k: int) -> int:
        k = int(k)
        if not 0 <= k < self.count:
            raise IndexError(f"element {k} of a list of {self.count}")  # IndexOutOfBounds
        return k


class _ElementReader(StructReader):
    """Element k of a list as a struct reader: StructListReader.get's result, or a pointer-list
    slot as a struct of one pointer. Reads are n = 1 read_elements_batch calls over the one element."""

    def __init__(self, lst: _ListReader, k: int, path=()):
        super().__init__(lst.reader.message, path, lst.reader.device)
        self._dev = lst.reader._framed()
        self.list, self.k = lst, k

    def _read(self, kind, offset, bit=0, what="StructReader"):
        d_in, off, ln = self._dev
        lst = self.list
        # element k alone: a table of one element whose head starts at element k
        h = lst.host_head.copy()
        h["elems_off"][0] += self.k * 8 * (int(h["data_words"][0]) + int(h["pointer_words"][0]))
        h["count"][0] = 1
        head = torch.from_numpy(h.view(np.uint8)).to(self.device)
        start = torch.tensor([0, 1], dtype=torch.int64, device=self.device)
        out = torch.zeros(3, dtype=torch.int64, device=self.device)
        st = torch.full((1,), -1, dtype=torch.int32, device=self.device)
        read_elements_batch(d_in, off, ln, head, start, lst.kind, 1, [Field(kind, offset, bit, self.path)],
                            out[0:1], out[1:2], st, out[2:3])
        _raise(int(st.item()), what)
        v, l, c = (int(x) for x in out.cpu().numpy().view(np.uint64))
        return v, l, c

    def read_struct(self, pointer_index: int) -> "StructReader":
        child = _ElementReader(self.list, self.k, self.path + (pointer_index,))
        child._read(FIELD_U8, 0, what="StructReader.readStruct")
        return child

    def _nested(self, pointer_index: int):
        raise InvalidArgument("a list inside a list element is not reachable: list_heads_batch starts at the root")

    read_struct_list = read_text_list = read_pointer_list = _nested


class StructListReader(_ListReader):
    """readStructList's result (message.zig:1165-1185, list_readers.zig:75-101)."""

    def get(self, k: int) -> StructReader:
        return _ElementReader(self, self._check(k))


class TextListReader(_ListReader):
    """readTextList's result (message.zig:1200-1210, list_readers.zig:103-144)."""

    def get(self, k: int) -> bytes:
        return _ElementReader(self, self._check(k)).read_text(0)


class PointerListReader(_ListReader):
    """readPointerList's result (message.zig:1212-1222, list_readers.zig:233-330)."""

    def _elem(self, k):
        return _ElementReader(self, self._check(k))

    def get_text(self, k: int) -> bytes:
        return self._elem(k).read_text(0)

    def get_data(self, k: int) -> bytes:
        return self._elem(k).read_data(0)

    def get_u16_list(self, k: int) -> list:
        return self._elem(k).read_u16_list(0)

    def get_u32_list(self, k: int) -> list:
        return self._elem(k).read_u32_list(0)

    def get_u64_list(self, k: int) -> list:
        return self._elem(k).read_u64_list(0)

    def get_struct(self, k: int) -> StructReader:
        return self._elem(k).read_struct(0)


def _read_struct_list(self, pointer_index: int) -> StructListReader:
    """readStructList (message.zig:1165-1185): one n = 1 list_heads_batch call."""
    return StructListReader(self, pointer_index, LIST_STRUCT, "StructReader.readStructList")


def _read_text_list(self, pointer_index: int) -> TextListReader:
    """readTextList (message.zig:1200-1210)."""
    return TextListReader(self, pointer_index, LIST_POINTER, "StructReader.readTextList")


def _read_pointer_list(self, pointer_index: int) -> PointerListReader:
    """readPointerList (message.zig:1212-1222)."""
    return PointerListReader(self, pointer_index, LIST_POINTER, "StructReader.readPointerList")


StructReader.read_struct_list = _read_struct_list
StructReader.read_text_list = _read_text_list
StructReader.read_pointer_list = _read_pointer_list


class Reader:
    """Mirror of Reader.init / Reader.initPacked (reader.zig:11-23)."""

    def __init__(self, msg: Message):
        self.msg = msg

    @classmethod
    def init(cls, data) -> "Reader":
        return cls(Message.init(data))

    @classmethod
    def init_packed(cls, data) -> "Reader":
        return cls(Message.init_packed(data))

    @staticmethod
    def read_packed_message(reader) -> bytes:
        """Reader.readPackedMessage (reader.zig:84-156): decode the packed message at
        the front of `reader` (bytes-like, or a binary file object with read/seek)
        and return its framed bytes, stopping at the length its segment table
        declares. A file object is left just past the message; on an error it is
        left where it was."""
        if hasattr(reader, "read"):
            start = reader.tell()
            data = reader.read()
            try:
                framed, used = read_packed_message_bytes(data)
            except PackedError:
                reader.seek(start)
                raise
            reader.seek(start + used)
            return framed
        return read_packed_message_bytes(reader)[0]


def read_packed_message_bytes(data) -> tuple:
    """(framed bytes, packed bytes consumed) of the message at the front of `data`
    (reader.zig:84-156), through the single-buffer C-ABI entry point."""
    data = bytes(data)
    src = _cbuf(data)
    cap = max(4096, 8 * len(data))
    for _ in range(2):  # a zero-run heavy message can expand past the first guess
        out = ctypes.create_string_buffer(cap)
        n, used = _sz(), _sz()
        st = lib().capnp_packed_read_message(src, len(data), out, cap, ctypes.byref(n), ctypes.byref(used))
        if st == OUT_OF_SPACE and n.value > cap:
            cap = n.value
            continue
        _raise(st, "readPackedMessage")
        return out.raw[:n.value], used.value
    raise OutOfSpace("readPackedMessage: framed length grew between calls")


# ---------------------------------------------------------------------------
# Framing for packed byte streams
# ---------------------------------------------------------------------------

_PIN_MIN = 1 << 20


def _host_bytes(nbytes: int, pin: bool = True) -> np.ndarray:
    """A host byte buffer for a framer call. With `pin`, from 1 MiB up it is page-locked memory
    from torch's caching host allocator: the session's H2D / D2H copies then run at the link's
    DMA rate instead of through the runtime's pageable staging, and a freed buffer (its last
    frame view dropped) goes back to torch's cache for the next read."""
    if pin and nbytes >= _PIN_MIN and torch is not None and torch.cuda.is_available():
        return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True).numpy()
    return np.empty(max(nbytes, 1), dtype=np.uint8)


class FramerSession:
    """A capnp_packed_framer: the Framer state of n connections kept on the device between
    reads (include/capnp_packed.h). Each connection's unconsumed packed bytes
    stay in device memory and the walk to the current message's end resumes where the last
    read left it, so a message split over k reads is uploaded once and walked once."""

    def __init__(self, n_conns: int):
        h = _vp()
        _raise(lib().capnp_packed_framer_create(int(n_conns), ctypes.byref(h)), "framer_create")
        self.handle, self.n = h, int(n_conns)

    def close(self):
        if getattr(self, "handle", None):
            lib().capnp_packed_framer_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    def read(self, reads: dict):
        """Append `reads` ({connection: bytes}) and pop every whole message. Returns
        (frames, status): frames[c] lists connection c's frames in order (read-only
        memoryviews of the call's frame buffers), status an int32 array: END_OF_STREAM, or the
        reader's error after which the connection's bytes were dropped."""
        gc_on = gc.isenabled()
        gc.disable()  # no cycles among the views; the collector's passes cost more
        try:
            return self._read(reads)
        finally:
            if gc_on:
                gc.enable()

    def assemble(self, reads: dict):
        """The connections' new bytes as one host buffer (page-locked from 1 MiB up) with
        per-connection offsets and lengths: the input of read_raw."""
        n = self.n
        lens = np.zeros(n, dtype=np.uint64)
        for c, d in reads.items():
            lens[c] = len(d)
        off = np.zeros(n, dtype=np.uint64)
        off[1:] = np.cumsum(lens)[:-1]
        host = _host_bytes(int(lens.sum()))
        for c, d in reads.items():
            if len(d):
                host[int(off[c]):int(off[c]) + len(d)] = np.frombuffer(d, dtype=np.uint8)
        return host, off, lens

    def read_raw(self, host, off, lens):
        """capnp_packed_framer_read over an assembled input (a server that receives into one
        buffer skips assemble()). Returns (parts, status): parts lists (buf, f_off, f_len,
        f_conn) per native call, frame i of a part being buf[f_off[i]:f_off[i] + f_len[i]] of
        connection f_conn[i], a connection's frames in order over the parts; status as read()."""
        total = int(lens.sum())

        def first(*out):
            return lib().capnp_packed_framer_read(self.handle, host.ctypes.data, total, off.ctypes.data,
                                                  lens.ctypes.data, *out)
        return self._pop(first, total)

    def readv_raw(self, reads: dict):
        """read_raw over the connections' own bytes objects (capnp_packed_framer_readv: the
        library gathers them into its page-locked staging, no host-side layout)."""
        n = self.n
        ptrs = (ctypes.c_char_p * n)()
        lens = np.zeros(n, dtype=np.uint64)
        keep = []
        for c, d in reads.items():
            if len(d):
                d = d if isinstance(d, bytes) else bytes(d)
                keep.append(d)  # alive through the call
                ptrs[c] = d
                lens[c] = len(d)
        total = int(lens.sum())

        def first(*out):
            return lib().capnp_packed_framer_readv(self.handle, ptrs, lens.ctypes.data, *out)
        return self._pop(first, total)

    def _pop(self, first_call, total: int):
        n = self.n
        status = np.zeros(n, dtype=np.int32)
        parts = []
        # frames of 2x the read's bytes: the buffer runs out only for messages packed below
        # half their size, and then the loop below pops the rest into a larger one
        cap, max_frames = max(1 << 16, 2 * total + (1 << 16)), max(1024, total // 2 + 64)
        first = True
        while True:
            # a retry's buffer is sized for one large message: pageable, as pinning it fresh
            # costs more than the runtime's staged copy of it
            buf = _host_bytes(cap, pin=first)
            f_off = np.empty(max_frames, dtype=np.uint64)
            f_len = np.empty(max_frames, dtype=np.uint64)
            f_conn = np.empty(max_frames, dtype=np.uint32)
            st_call = np.zeros(n, dtype=np.int32)
            nf = ctypes.c_uint32(0)
            out = (buf.ctypes.data, cap, f_off.ctypes.data, f_len.ctypes.data, f_conn.ctypes.data, max_frames,
                   st_call.ctypes.data, ctypes.byref(nf))
            if first:
                rc = first_call(*out)
            else:  # later calls pop what is held, no new bytes
                rc = lib().capnp_packed_framer_read(self.handle, None, 0, None, None, *out)
            if rc not in (OK, OUT_OF_SPACE):
                try:
                    _raise(rc, "framer_read")
                except PackedError as exc:
                    # the session already advanced past the frames of earlier calls of this read:
                    # hand them over with the error instead of losing them (exc.partial, as read_raw
                    # returns them: (parts, status))
                    status[status == 0] = END_OF_STREAM
                    exc.partial = (parts, status)
                    raise
            first = False
            err = st_call != END_OF_STREAM
            status[err] = st_call[err]
            k = nf.value
            if k:
                parts.append((buf, f_off[:k], f_len[:k], f_conn[:k]))
            if rc == OK:
                break
            # frames or the table filled up: pop the rest into larger ones; a buffer of the
            # largest known framed length pops at least that message
            big = max((self.expected(c) for c in range(n)), default=0)
            cap = max(cap * 2 if k == 0 else cap, (big + 7) // 8 * 8 + 64)
            max_frames *= 2
        status[status == 0] = END_OF_STREAM
        return parts, status

    def _read(self, reads: dict):
        try:
            parts, status = self.readv_raw(reads)
        except PackedError as exc:
            if hasattr(exc, "partial"):  # frames popped before the failing call: exc.frames
                exc.frames = self._group(*exc.partial)[0]
            raise
        return self._group(parts, status)

    @staticmethod
    def _group(parts, status):
        frames = {}
        for buf, f_off, f_len, f_conn in parts:
            # a connection's frames are in order within a call: group them by a stable sort
            view = memoryview(buf).toreadonly()
            if len(f_conn) > 1 and bool((f_conn[1:] < f_conn[:-1]).any()):  # a later pass's frames
                order = np.argsort(f_conn, kind="stable")
                conn_s, fo, fl = f_conn[order], f_off[order], f_len[order]
            else:  # one walk pass: already grouped by connection, in order
                conn_s, fo, fl = f_conn, f_off, f_len
            fo_l, fe_l = fo.tolist(), (fo + fl).tolist()
            cuts = (np.flatnonzero(np.diff(conn_s)) + 1).tolist()
            starts = [0] + cuts
            for c, a, b in zip(conn_s[starts].tolist(), starts, cuts + [len(conn_s)]):
                frames.setdefault(c, []).extend(map(view.__getitem__, map(slice, fo_l[a:b], fe_l[a:b])))
        return frames, status

    def buffered(self, c: int) -> int:
        b = ctypes.c_uint64()
        _raise(lib().capnp_packed_framer_buffered(self.handle, int(c), ctypes.byref(b)), "framer_buffered")
        return b.value

    def expected(self, c: int) -> int:
        """Framer.expected_total (framing.zig:10): framed bytes of connection c's current
        message once its header is decoded, else 0."""
        b = ctypes.c_uint64()
        _raise(lib().capnp_packed_framer_expected(self.handle, int(c), ctypes.byref(b)), "framer_expected")
        return b.value

    def reset(self, c: int) -> None:
        _raise(lib().capnp_packed_framer_reset(self.handle, int(c)), "framer_reset")

    def stats(self) -> dict:
        up, mv = ctypes.c_uint64(), ctypes.c_uint64()
        _raise(lib().capnp_packed_framer_stats(self.handle, ctypes.byref(up), ctypes.byref(mv)), "framer_stats")
        return {"uploaded_bytes": up.value, "moved_bytes": mv.value}

    def walk_stats(self) -> dict:
        """Walk passes run and the windows they built lookup tables for."""
        ps, tw = ctypes.c_uint64(), ctypes.c_uint64()
        _raise(lib().capnp_packed_framer_walk_stats(self.handle, ctypes.byref(ps), ctypes.byref(tw)),
               "framer_walk_stats")
        return {"passes": ps.value, "table_windows": tw.value}


class PackedFramer:
    """The RPC `Framer` (src/rpc/level0/framing.zig:4-90) for a PACKED byte stream.
    It has the same surface: push / buffered_bytes / reset / pop_frame.
    - push() appends a socket read.
    - pop_frame() returns the framed (unpacked) bytes of the next whole message, or None
      while the buffered bytes do not hold one yet (the reader's EndOfStream).
    - pop_frame() raises the reader's other errors (reader.zig:84-156). The caller then
      reset()s, as Connection.handleRead does (level2/connection.zig:175-184).
    - A message's end is only known by decoding its packed records, so the buffered bytes
      live on the device (a one-connection FramerSession): a push's bytes are uploaded once,
      and the walk to the message end resumes where the previous pop left it.
    - PackedConnections does this for many connections at once."""

    max_frame_words = 8 * 1024 * 1024  # framing.zig:5 / reader.zig:6
    max_segment_count = MAX_SEGMENT_COUNT

    def __init__(self):
        self.session = FramerSession(1)
        self.pending = []      # pushed bytes not yet handed to the session
        self.ready = deque()   # frames popped from the device (then the error that ended them)
        self.error = None      # the framing error once raised: raised again until reset()

    def push(self, data) -> None:
        if len(data):
            self.pending.append(bytes(data))

    def buffered_bytes(self) -> int:
        """Framer.bufferedBytes (framing.zig:30-32): pushed bytes not yet framed. One difference:
        pop_frame takes every whole message off the device at once, and the packed bytes of the
        frames it holds for later pop_frame calls are no longer counted (the device does not
        report each frame's packed length)."""
        return self.session.buffered(0) + sum(len(d) for d in self.pending)

    def reset(self) -> None:
        self.session.reset(0)
        self.pending.clear()
        self.ready.clear()
        self.error = None

    def pop_frame(self):
        if self.error is not None:  # framing.zig: the corrupt bytes keep failing until reset
            raise self.error
        if not self.ready and self.pending:
            data = b"".join(self.pending)
            self.pending.clear()
            frames, status = self.session.read({0: data})
            self.ready.extend(bytes(f) for f in frames.get(0, []))
            if int(status[0]) != END_OF_STREAM:
                rs = int(status[0])
                self.ready.append(_ERRORS.get(rs, DeviceError)(
                    f"readPackedMessage: {lib().capnp_packed_status_name(rs).decode()}"))
        if not self.ready:
            return None
        v = self.ready.popleft()
        if isinstance(v, Exception):
            self.error = v
            raise v
        return v


class _ConnView:
    """A PackedConnections connection's framer surface (bufferedBytes / reset)."""

    def __init__(self, session, c):
        self._s, self._c = session, c

    def buffered_bytes(self) -> int:
        return self._s.buffered(self._c)

    def reset(self) -> None:
        self._s.reset(self._c)


class PackedConnections:
    """Connection.handleRead (src/rpc/level2/connection.zig:153-203) over many
    connections at once, on one FramerSession: every connection's Framer state (its
    unconsumed packed bytes, the current message's framed length, where the walk to its end
    stopped) stays on the device between reads.
    - handle_read(reads) uploads only the new bytes and pops every whole message in one
      native call (capnp_packed_framer_read).
    - Per connection, the result is the list of frames popped (in order), or a PackedError.
    - On the error the connection's framer is reset and the connection is closed for
      further reads, as handleRead does (175-184). Frames popped before the error are
      dropped with it; handleRead would already have delivered them, so
      `frames_before_error` keeps them.
    - A connection whose bytes end inside a message keeps them for its next read (the
      reader's EndOfStream = popFrame's null), and its walk resumes there."""

    def __init__(self, n_conns: int, device="cuda"):
        self.session = FramerSession(n_conns)
        self.framers = [_ConnView(self.session, c) for c in range(n_conns)]
        self.closed = [False] * n_conns
        self.frames_before_error = {}
        self.device = torch.device(device)

    def handle_read(self, reads: dict) -> dict:
        """One native call: the connections' new bytes go to the device once, every whole
        message is popped, and the frames come back as read-only memoryviews of the call's
        frame buffer (no per-frame copy; the buffer lives as long as its frames)."""
        gc_on = gc.isenabled()
        gc.disable()  # the result's lists and views hold no cycles
        try:
            return self._handle_read(reads)
        finally:
            if gc_on:
                gc.enable()

    def _handle_read(self, reads: dict) -> dict:
        live = {c: d for c, d in reads.items() if not self.closed[c] and len(d)}
        frames, status = self.session.read(live)
        result = {c: [] for c in live}
        result.update(frames)
        for c in np.nonzero(status != END_OF_STREAM)[0].tolist():
            rs = int(status[c])
            self.frames_before_error[c] = result.get(c, [])
            result[c] = _ERRORS.get(rs, DeviceError)(f"readPackedMessage: {lib().capnp_packed_status_name(rs).decode()}")
            self.closed[c] = True
        return result


# ---------------------------------------------------------------------------
# device-resident batch API (torch tensors in HBM)
# ---------------------------------------------------------------------------

def set_decoder(name: str) -> str:
    """Select the mid-unit batch decoder ("auto", "twopass", "words"; "fused" and "stream" were
    removed in round 5 and raise) for batches enqueued from now on; returns the previous
    setting's name. Every one is bit-exact."""
    prev = lib().capnp_packed_set_decoder(DECODERS[name])
    if prev < 0 or prev not in DECODERS.values():
        _raise(prev, "set_decoder")
    return {v: k for k, v in DECODERS.items()}[prev]


def decoder_available(name: str) -> bool:
    """Whether this build has the decoder: "auto", "twopass" and "words"; not "fused" and
    "stream" (removed in round 5)."""
    L = lib()
    prev = L.capnp_packed_set_decoder(DECODERS[name])
    if prev not in DECODERS.values():
        return False
    L.capnp_packed_set_decoder(prev)
    return True


def set_all_or_nothing(on: bool) -> bool:
    """Small decode units all-or-nothing too (capnp_packed_set_all_or_nothing); returns the
    previous setting."""
    return bool(lib().capnp_packed_set_all_or_nothing(1 if on else 0))


def set_launch_flags(flags: int) -> int:
    """Launch policy bits (capnp_packed_set_launch_flags: LAUNCH_LONG_INLINE,
    LAUNCH_MID_SIDE_STREAM, LAUNCH_CLASS_SCAN); returns the previous flags. No result depends on them."""
    return int(lib().capnp_packed_set_launch_flags(int(flags)))


class launch_flags:
    """Context manager: `with launch_flags(LAUNCH_LONG_INLINE): ...` restores the flags after."""

    def __init__(self, flags: int):
        self.flags, self.prev = flags, None

    def __enter__(self):
        self.prev = set_launch_flags(self.flags)
        return self

    def __exit__(self, *exc):
        set_launch_flags(self.prev)
        return False


class decoder:
    """Context manager: `with decoder("words"): ...` restores the previous decoder after."""

    def __init__(self, name: str):
        self.name, self.prev = name, None

    def __enter__(self):
        self.prev = set_decoder(self.name)
        return self

    def __exit__(self, *exc):
        set_decoder(self.prev)
        return False


def stream_release(stream=None) -> None:
    """Free the library's context of a stream (side stream, events, queues); see
    capnp_packed_stream_release. Synchronises the stream."""
    _raise(lib().capnp_packed_stream_release(_stream(stream)), "stream_release")


def stream_queue_info(stream=None):
    """(bytes of the stream's queue, replaced queues kept for captured graphs)."""
    b, k = ctypes.c_size_t(), ctypes.c_uint32()
    _raise(lib().capnp_packed_stream_queue_info(_stream(stream), ctypes.byref(b), ctypes.byref(k)),
           "stream_queue_info")
    return b.value, k.value


def stream_contexts() -> int:
    """How many caller streams the library holds a context for (capnp_packed_stream_contexts)."""
    k = ctypes.c_uint32()
    _raise(lib().capnp_packed_stream_contexts(ctypes.byref(k)), "stream_contexts")
    return k.value


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _stream(stream) -> int:
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)


def _units(in_off, *per_unit) -> int:
    """Unit count of a batch (in_off's length); every per-unit tensor must hold at
    least that many entries (the kernels index them by unit)."""
    n = in_off.numel()
    for t in per_unit:
        if t is not None and t.numel() < n:
            raise InvalidArgument(f"per-unit tensor has {t.numel()} entries for {n} units")
    return n


def _ws_tensor(nbytes: int, device):
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)


def workspace(n_units: int, device="cuda"):
    """Device workspace for the *_batch_ws calls (capnp_packed_batch_workspace_bytes):
    a batch that uses its own workspace shares no library state, so a captured
    hipGraph of it may replay beside any other work."""
    return _ws_tensor(lib().capnp_packed_batch_workspace_bytes(n_units), device)


def _ws(ws):
    return (0, 0) if ws is None else (ws.data_ptr(), ws.numel() * ws.element_size())


def encode_batch(d_in, in_off, in_len, d_out, out_off, out_cap, out_len, status, stream=None, ws=None,
                 dialect="zig") -> None:
    """Batch packPacked: unit i = d_in[in_off[i] : in_off[i]+in_len[i]] -> slot
    d_out[out_off[i] : out_off[i]+out_cap[i]]; out_len[i], status[i] per unit.
    ws: optional workspace() tensor (capnp_packed_encode_batch_ws).
    dialect="cxx": every unit as one piece under the C++ rule (capnp_packed_encode_batch_dialect)."""
    d = _dialect(dialect)
    n = _units(in_off, in_len, out_off, out_cap, out_len, status)
    if d != 0:
        if d_out is None:
            raise InvalidArgument("encode_batch needs an output buffer (sizes only: encoded_size_batch)")
        _raise(lib().capnp_packed_encode_batch_dialect(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out),
                                                       _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                                       d, *_ws(ws), _stream(stream)), "encode_batch_dialect")
    elif ws is None:
        _raise(lib().capnp_packed_encode_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out),
                                               _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                               _stream(stream)), "encode_batch")
    else:
        _raise(lib().capnp_packed_encode_batch_ws(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out),
                                                  _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                                  *_ws(ws), _stream(stream)), "encode_batch_ws")


def dense_workspace(n_units: int, device="cuda"):
    """Device workspace of encode_dense_batch (capnp_packed_encode_dense_workspace_bytes); the
    call zeroes it itself. Two calls in flight must not share one."""
    return _ws_tensor(lib().capnp_packed_encode_dense_workspace_bytes(n_units), device)


def encode_dense_batch(d_in, in_off, in_len, d_out, out_off, out_len, status, base=0, cap=None, stream=None,
                       ws=None, dialect="zig") -> None:
    """Batch writePackedTo on one writer (capnp_packed_encode_dense_batch): the units packed
    back to back into d_out[base ..) in unit order, in one pass. out_off (n + 1 entries) gets
    the running offsets (out_off[0] = base, out_off[n] = the stream's end), out_len / status
    are per unit. cap: the stream may use d_out[0 : cap) (None: all of d_out); a unit that
    would end past it is not written and gets OUT_OF_SPACE, the offsets go on. d_out=None:
    sizes and offsets only. ws: a dense_workspace() tensor (None: one is allocated for the call)."""
    _encode_dense("encode_dense_batch", d_in, in_off, in_len, d_out, out_off, out_len, status, base, cap, stream, ws,
                  dialect)


def _encode_dense(name, d_in, in_off, in_len, d_out, out_off, out_len, status, base, cap, stream, ws, dialect):
    """encode_dense_batch / encode_framed_dense_batch through the library's capnp_packed_<name>."""
    d = _dialect(dialect)
    n = _units(in_off, in_len, out_len, status)
    if out_off is not None and out_off.numel() < n + 1:
        raise InvalidArgument(f"out_off has {out_off.numel()} entries for {n} units (n + 1 needed)")
    if cap is None:
        cap = 0 if d_out is None else d_out.numel()
    if ws is None and n:
        ws = dense_workspace(n, device=in_off.device)
    fn = getattr(lib(), "capnp_packed_" + name)
    _raise(fn(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out), base, cap, _ptr(out_off), _ptr(out_len),
              _ptr(status), d, *_ws(ws), _stream(stream)), name)


def framed_workspace(n_units: int, device="cuda"):
    """Device workspace of encode_framed_batch (capnp_packed_encode_framed_workspace_bytes). Two
    calls in flight must not share one."""
    return _ws_tensor(lib().capnp_packed_encode_framed_workspace_bytes(n_units), device)


def encode_framed_batch(d_in, in_off, in_len, d_out, out_off, out_cap, out_len, status, stream=None, ws=None,
                        dialect="zig") -> None:
    """encode_batch over framed messages (capnp_packed_encode_framed_batch): every unit is checked
    as one whole framed message (the table errors, TRUNCATED_MESSAGE, INVALID_ARGUMENT for trailing
    words; a failed unit's slot stays untouched), and dialect="cxx" packs its segment table and
    each segment as pieces of their own. d_out=None: sizes only. ws: a framed_workspace() tensor
    (None: one is allocated for the call)."""
    d = _dialect(dialect)
    n = _units(in_off, in_len, out_len, status)
    if d_out is not None:
        _units(in_off, out_off, out_cap)
    if ws is None and n:
        ws = framed_workspace(n, device=in_off.device)
    _raise(lib().capnp_packed_encode_framed_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out),
                                                  _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status), d,
                                                  *_ws(ws), _stream(stream)), "encode_framed_batch")


def encode_framed_dense_batch(d_in, in_off, in_len, d_out, out_off, out_len, status, base=0, cap=None, stream=None,
                              ws=None, dialect="zig") -> None:
    """encode_dense_batch over framed messages (capnp_packed_encode_framed_dense_batch): the batch
    form of writing message after message to one packed stream; with dialect="cxx" the stream is
    byte for byte what capnp convert binary:packed writes. A failed unit takes no bytes. ws: a
    dense_workspace() tensor (None: one is allocated for the call)."""
    _encode_dense("encode_framed_dense_batch", d_in, in_off, in_len, d_out, out_off, out_len, status, base, cap,
                  stream, ws, dialect)


def write_packed_messages(frames, dialect="zig", device="cuda") -> bytes:
    """The packed stream of a list of framed messages, the writer's half of read_packed_messages:
    one upload of the frames end to end, one encode_framed_dense_batch, one download of the
    stream. Raises the first failed frame's error, with that frame's index."""
    _dialect(dialect)
    frames = [bytes(f) for f in frames]
    if not frames:
        return b""
    dev = torch.device(device)
    n = len(frames)
    # every frame starts on a word: a frame whose length is no multiple of 8 (its own error)
    # must not misalign the next
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    starts = np.concatenate(([0], np.cumsum((lens + 7) & ~7)[:-1])).astype(np.int64)
    host = np.zeros(int(((lens + 7) & ~7).sum()) + 16, dtype=np.uint8)
    for s, f in zip(starts.tolist(), frames):
        host[s:s + len(f)] = np.frombuffer(f, dtype=np.uint8)
    d_in = torch.from_numpy(host).to(dev)
    in_off = torch.from_numpy(starts).to(dev)
    in_len = torch.from_numpy(lens).to(dev)
    cap = encode_bound(int(host.size))
    d_out = torch.empty(max(cap, 1), dtype=torch.uint8, device=dev)
    out_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    out_len = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    encode_framed_dense_batch(d_in, in_off, in_len, d_out, out_off, out_len, status, cap=cap, dialect=dialect)
    st = status.cpu().numpy()
    bad = np.flatnonzero(st != OK)
    if bad.size:
        _raise(int(st[bad[0]]), f"write_packed_messages: frame {int(bad[0])}")
    return d_out[:int(out_off[n].item())].cpu().numpy().tobytes()


def encoded_size_batch(d_in, in_off, in_len, out_len, status, stream=None, dialect="zig") -> None:
    d = _dialect(dialect)
    n = _units(in_off, in_len, out_len, status)
    if d != 0:
        _raise(lib().capnp_packed_encode_batch_dialect(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, 0, 0, 0,
                                                       _ptr(out_len), _ptr(status), d, 0, 0, _stream(stream)),
               "encoded_size_batch_dialect")
        return
    _raise(lib().capnp_packed_encoded_size_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(out_len),
                                                 _ptr(status), _stream(stream)), "encoded_size_batch")


def decode_batch(d_in, in_off, in_len, d_out, out_off, out_cap, out_len, status, stream=None, ws=None) -> None:
    """Batch unpackPacked: unit i = d_in[in_off[i] : in_off[i]+in_len[i]] -> slot
    d_out[out_off[i] : out_off[i]+out_cap[i]]; out_len[i], status[i] per unit.
    ws: optional workspace() tensor (capnp_packed_decode_batch_ws)."""
    n = _units(in_off, in_len, out_off, out_cap, out_len, status)
    if ws is None:
        _raise(lib().capnp_packed_decode_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out),
                                               _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                               _stream(stream)), "decode_batch")
    else:
        _raise(lib().capnp_packed_decode_batch_ws(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out),
                                                  _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                                  *_ws(ws), _stream(stream)), "decode_batch_ws")


def decoded_size_batch(d_in, in_off, in_len, out_len, status, stream=None) -> None:
    n = _units(in_off, in_len, out_len, status)
    _raise(lib().capnp_packed_decoded_size_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(out_len),
                                                 _ptr(status), _stream(stream)), "decoded_size_batch")


def read_message_batch(d_in, in_off, in_len, d_out, out_off, out_cap, out_len, consumed, status,
                       stream=None) -> None:
    """Batch Reader.readPackedMessage (reader.zig:84-156): one message from the front
    of each unit (a reader's buffered packed stream) -> its slot; consumed[i] =
    packed bytes the message took (0 on error), out_len[i] = framed bytes."""
    n = _units(in_off, in_len, out_off, out_cap, out_len, consumed, status)
    _raise(lib().capnp_packed_read_message_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(d_out),
                                                 _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(consumed),
                                                 _ptr(status), _stream(stream)), "read_message_batch")


def split_workspace(n: int, in_bytes_bound: int, device="cuda"):
    """Device workspace of split_streams (capnp_packed_split_workspace_bytes) for n streams of
    at most in_bytes_bound packed bytes in all; the call sets it up itself. The bound sizes the
    window tables only: a smaller one (0 included) costs time on long streams, never results.
    Two calls in flight must not share one."""
    return _ws_tensor(lib().capnp_packed_split_workspace_bytes(n, in_bytes_bound), device)


def split_streams(d_in, in_off, in_len, msg_first, msg_off, msg_len, msg_framed, consumed, status,
                  msg_stream=None, ws=None, stream=None) -> None:
    """Dense streams of packed messages split into their messages (capnp_packed_split_streams):
    stream s = d_in[in_off[s] : in_off[s] + in_len[s]] is what repeated Reader.readPackedMessage
    calls on one reader would consume. msg_first (n + 1 entries) gets the whole messages before
    each stream (msg_first[n]: the total); row k of the tables (msg_off.numel() rows; rows past
    that are counted, not written) gets the message's offset in d_in, its packed and its framed
    length, msg_stream[k] (int32, optional) its stream. consumed / status are per stream.
    (msg_off, msg_len) are a decode_batch's or read_message_batch's (in_off, in_len);
    lengths_to_offsets(msg_framed) its dense output layout. msg_off / msg_len / msg_framed may
    all be None (counts only). ws: a split_workspace() tensor (None: one without window tables
    is allocated for the call)."""
    n = _units(in_off, in_len, consumed, status)
    if msg_first is None or msg_first.numel() < n + 1:
        raise InvalidArgument(f"msg_first needs {n + 1} entries for {n} streams")
    tables = (msg_off, msg_len, msg_framed)
    if any(t is None for t in tables) and not all(t is None for t in tables):
        raise InvalidArgument("msg_off, msg_len and msg_framed go together")
    max_msgs = 0 if msg_off is None else min(t.numel() for t in tables)
    if msg_stream is not None and msg_stream.numel() < max_msgs:
        raise InvalidArgument(f"msg_stream has {msg_stream.numel()} entries for {max_msgs} rows")
    if ws is None and n:
        ws = split_workspace(n, 0, device=in_off.device)
    _raise(lib().capnp_packed_split_streams(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, max_msgs, _ptr(msg_first),
                                            _ptr(msg_off), _ptr(msg_len), _ptr(msg_framed), _ptr(msg_stream),
                                            _ptr(consumed), _ptr(status), *_ws(ws), _stream(stream)),
           "split_streams")


def read_packed_messages(data, device="cuda") -> tuple:
    """Every whole message of a host packed stream: (frames, consumed, status_name), what calling
    Reader.readPackedMessage on one reader until it fails or runs dry gives. frames: the framed
    bytes of the whole messages in order; consumed: their packed bytes; status_name: "OK" when
    every byte was consumed, else the name of the status the loop stopped with (the frames
    before it are still returned). One upload of the bytes, split_streams -> lengths_to_offsets
    -> decode_batch on the device, one download of all frames (plus the two totals that size
    the tables and the download)."""
    data = bytes(data)
    if not data:
        return [], 0, lib().capnp_packed_status_name(OK).decode()
    dev = torch.device(device)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    in_off = torch.zeros(1, dtype=torch.int64, device=dev)
    in_len = torch.full((1,), len(data), dtype=torch.int64, device=dev)
    first = torch.empty(2, dtype=torch.int64, device=dev)
    consumed = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = split_workspace(1, len(data), device=dev)
    rows = len(data) // 64 + 16  # a first guess; msg_first[1] is the count a retry needs
    while True:
        tab = torch.empty((3, rows), dtype=torch.int64, device=dev)
        split_streams(d_in, in_off, in_len, first, tab[0], tab[1], tab[2], consumed, status, ws=ws)
        total = int(first[1].item())
        if total <= rows:
            break
        rows = total
    st_name = lib().capnp_packed_status_name(int(status.item())).decode()
    used = int(consumed.item())
    if total == 0:
        return [], used, st_name
    framed = tab[2][:total]
    out_off = lengths_to_offsets(framed)
    nbytes = int(out_off[total].item())
    d_out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out_len = torch.empty(total, dtype=torch.int64, device=dev)
    dst = torch.empty(total, dtype=torch.int32, device=dev)
    decode_batch(d_in, tab[0][:total], tab[1][:total], d_out, out_off, framed, out_len, dst)
    host = d_out.cpu().numpy().tobytes()
    bad = int((dst != OK).sum().item())
    if bad:
        raise DeviceError(f"read_packed_messages: {bad} of {total} split messages failed to decode")
    ends = out_off.cpu().tolist()
    return [host[ends[k]:ends[k + 1]] for k in range(total)], used, st_name


def encode_message_batch(seg_ptr, seg_len, seg_first, seg_count, d_out, out_off, out_cap, out_len, status,
                         stream=None, dialect="zig") -> None:
    """MessageBuilder.toPackedBytes (message.zig:2123-2179) for a batch of messages,
    packed straight from their segments. seg_ptr / seg_len: int64 tensors of segment
    device addresses and byte lengths; seg_first / seg_count: int32 tensors, one
    entry per message. d_out None = packed sizes only. dialect="cxx": the C++ message
    writer's bytes (the segment table and each segment packed as pieces of their own)."""
    d = _dialect(dialect)
    n = _units(seg_first, seg_count, out_len, status)
    if d_out is not None:
        _units(seg_first, out_off, out_cap)
    if d != 0:
        _raise(lib().capnp_packed_encode_message_batch_dialect(
            _ptr(seg_ptr), _ptr(seg_len), _ptr(seg_first), _ptr(seg_count), n, _ptr(d_out), _ptr(out_off),
            _ptr(out_cap), _ptr(out_len), _ptr(status), d, _stream(stream)), "encode_message_batch_dialect")
        return
    _raise(lib().capnp_packed_encode_message_batch(_ptr(seg_ptr), _ptr(seg_len), _ptr(seg_first), _ptr(seg_count),
                                                   n, _ptr(d_out), _ptr(out_off), _ptr(out_cap), _ptr(out_len),
                                                   _ptr(status), _stream(stream)), "encode_message_batch")


def pack_message_cxx(segments, device="cuda") -> bytes:
    """One message's packed bytes under the C++ dialect, from host segments: they are
    uploaded end to end and packed by encode_message_batch(dialect="cxx")."""
    segs = [bytes(s) for s in segments] or [b""]
    if len(segs) > MAX_SEGMENT_COUNT:
        raise InvalidArgument(f"{len(segs)} segments (at most {MAX_SEGMENT_COUNT})")
    for s in segs:
        if len(s) % 8:
            raise InvalidMessageSize("segment length is not a multiple of 8")
    lens = np.array([len(s) for s in segs], dtype=np.int64)
    total = int(lens.sum())
    data = torch.from_numpy(np.frombuffer(b"".join(segs) + bytes(8), dtype=np.uint8).copy()).to(device)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
    seg_ptr = torch.from_numpy(offs + data.data_ptr()).to(device)
    seg_len = torch.from_numpy(lens).to(device)
    first = torch.zeros(1, dtype=torch.int32, device=device)
    count = torch.full((1,), len(segs), dtype=torch.int32, device=device)
    cap = encode_bound(8 * (len(segs) // 2 + 1) + total)
    out = torch.empty(max(cap, 1), dtype=torch.uint8, device=device)
    off = torch.zeros(1, dtype=torch.int64, device=device)
    capt = torch.full((1,), cap, dtype=torch.int64, device=device)
    ln = torch.zeros(1, dtype=torch.int64, device=device)
    st = torch.full((1,), -1, dtype=torch.int32, device=device)
    encode_message_batch(seg_ptr, seg_len, first, count, out, off, capt, ln, st, dialect="cxx")
    _raise(int(st.item()), "toPackedBytes")
    return out[:int(ln.item())].cpu().numpy().tobytes()


def message_init_batch(d_in, in_off, in_len, max_segs, seg_count, seg_off, seg_len, status, stream=None) -> None:
    """Message.init (message.zig:341-394) segment tables of a batch of framed messages:
    seg_count[i] (int32), seg_off / seg_len rows of max_segs entries (int64)."""
    n = _units(in_off, in_len, seg_count, status)
    if max_segs and (seg_off.numel() < n * max_segs or seg_len.numel() < n * max_segs):
        raise InvalidArgument("segment tables need n * max_segs entries")
    _raise(lib().capnp_packed_message_init_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, max_segs,
                                                 _ptr(seg_count), _ptr(seg_off), _ptr(seg_len), _ptr(status),
                                                 _stream(stream)), "message_init_batch")


# Message.ValidationOptions defaults (message.zig:331-335)
DEFAULT_SEGMENT_COUNT_LIMIT = MAX_SEGMENT_COUNT
DEFAULT_TRAVERSAL_LIMIT_WORDS = 8 * 1024 * 1024
DEFAULT_NESTING_LIMIT = 64


def validate_batch(d_in, in_off, in_len, status, words=None, segment_count_limit=DEFAULT_SEGMENT_COUNT_LIMIT,
                   traversal_limit_words=DEFAULT_TRAVERSAL_LIMIT_WORDS, nesting_limit=DEFAULT_NESTING_LIMIT,
                   stream=None) -> None:
    """Message.validate (message.zig:699-969) of a batch of framed messages (the bytes
    Message.init takes): status[i] = 0 or the reference's first error for message i;
    words[i] (optional int64) = traversal words the walk consumed (0 on error).
    Any nesting limit is accepted; the device applies at most 2^18 (the C-ABI takes a u32,
    so larger values are clamped here first)."""
    n = _units(in_off, in_len, status, words)
    nesting_limit = min(int(nesting_limit), 0xFFFFFFFF)
    _raise(lib().capnp_packed_validate_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, segment_count_limit,
                                             traversal_limit_words, nesting_limit, _ptr(status), _ptr(words),
                                             _stream(stream)), "validate_batch")


# capnp_packed_read_fields_batch kinds (include/capnp_packed.h)
FIELD_U8, FIELD_U16, FIELD_U32, FIELD_U64, FIELD_BOOL = 0, 1, 2, 3, 4
FIELD_TEXT, FIELD_DATA, FIELD_LIST_BIT, FIELD_LIST_16, FIELD_LIST_32, FIELD_LIST_64 = 5, 6, 7, 8, 9, 10
MAX_FIELDS = 32
MAX_PATH = 4


class CField(ctypes.Structure):
    """struct capnp_packed_field"""
    _fields_ = [("kind", ctypes.c_uint32), ("offset", ctypes.c_uint32), ("bit", ctypes.c_uint32),
                ("path_len", ctypes.c_uint32), ("path", ctypes.c_uint32 * 4)]


class Field:
    """One column of read_fields_batch: a kind, a byte offset in the data section (data kinds) or
    a pointer index (slice kinds), BOOL's bit, and the pointer indices of the readStruct steps
    from the root to the struct the field is read from."""

    def __init__(self, kind: int, offset: int, bit: int = 0, path=()):
        self.kind, self.offset, self.bit, self.path = int(kind), int(offset), int(bit), tuple(int(p) for p in path)

    def __repr__(self):
        return f"Field(kind={self.kind}, offset={self.offset}, bit={self.bit}, path={self.path})"

    def c(self) -> CField:
        # a path longer than the descriptor holds keeps its length, so the library refuses it
        padded = (self.path + (0,) * MAX_PATH)[:MAX_PATH]
        return CField(self.kind, self.offset, self.bit, len(self.path), (ctypes.c_uint32 * 4)(*padded))


def _cfields(fields):
    arr = (CField * max(1, len(fields)))()
    for i, f in enumerate(fields):
        arr[i] = f.c()
    return arr


def _check_field_major(columns, nf, rows, what):
    for t in columns:
        if t is not None and t.numel() < rows * nf:
            raise InvalidArgument(f"field-major output has {t.numel()} entries for {nf} fields x {rows} {what}")


def _check_head(head, n):
    if head is not None and head.numel() * head.element_size() < n * LIST_HEAD_BYTES:
        raise InvalidArgument(f"head holds {head.numel() * head.element_size()} bytes for {n} messages")


def read_fields_batch(d_in, in_off, in_len, fields, value, length, status, count=None, stream=None) -> None:
    """getRootStruct + StructReader reads (message.zig:973-985, :1010-1443) of a batch of framed
    messages as columns: entry f * n + i of value / length / count (int64) and status (int32) is
    field f of message i. A slice kind's value is the content's byte offset from d_in, so
    (value, length) columns feed gather_batch unchanged."""
    n = _units(in_off, in_len)
    nf = len(fields)
    _check_field_major((value, length, status, count), nf, n, "messages")
    arr = _cfields(fields)  # read by the call itself (passed to the kernel by value): free after it
    _raise(lib().capnp_packed_read_fields_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n,
                                                ctypes.addressof(arr), nf, _ptr(value), _ptr(length),
                                                _ptr(count), _ptr(status), _stream(stream)), "read_fields_batch")


def gather_batch(d_in, src_off, src_len, d_out, dst_off, status, cap=None, stream=None) -> None:
    """Row i = d_in[src_off[i] : src_off[i] + src_len[i]] copied to d_out[dst_off[i]:], byte-exact
    at any alignment; a row that would end past cap (default: d_out's size) gets OUT_OF_SPACE."""
    n = _units(src_off, src_len, dst_off, status)
    cap = d_out.numel() * d_out.element_size() if cap is None else int(cap)
    _raise(lib().capnp_packed_gather_batch(_ptr(d_in), _ptr(src_off), _ptr(src_len), n, _ptr(d_out), _ptr(dst_off),
                                           cap, _ptr(status), _stream(stream)), "gather_batch")


# capnp_packed_build_fields_batch (include/capnp_packed.h)
BUILD_STRUCT = 16
BUILD_ABSENT = 0xFFFFFFFFFFFFFFFF
MAX_BUILD_OPS = 32
MAX_BUILD_WORDS = 64


class CBuildOp(ctypes.Structure):
    """struct capnp_packed_build_op"""
    _fields_ = [("kind", ctypes.c_uint32), ("target", ctypes.c_uint32), ("offset", ctypes.c_uint32),
                ("bit", ctypes.c_uint32), ("data_words", ctypes.c_uint16), ("pointer_words", ctypes.c_uint16),
                ("reserved", ctypes.c_uint32 * 3)]


class BuildOp:
    """One builder call of build_fields_batch: a FIELD_* kind as a write, or BUILD_STRUCT
    (op 0: allocateStruct, later: initStruct). target is the BUILD_STRUCT op written into;
    offset is a byte offset in its data section (data kinds) or a pointer index."""

    def __init__(self, kind: int, offset: int, bit: int = 0, target: int = 0, data_words: int = 0,
                 pointer_words: int = 0):
        self.kind, self.offset, self.bit, self.target = int(kind), int(offset), int(bit), int(target)
        self.data_words, self.pointer_words = int(data_words), int(pointer_words)

    def __repr__(self):
        return (f"BuildOp(kind={self.kind}, offset={self.offset}, bit={self.bit}, target={self.target}, "
                f"data_words={self.data_words}, pointer_words={self.pointer_words})")

    def c(self) -> CBuildOp:
        return CBuildOp(self.kind, self.target, self.offset, self.bit, self.data_words, self.pointer_words,
                        (ctypes.c_uint32 * 3)(0, 0, 0))


def build_fields_batch(d_pool, ops, value, length, d_out, out_off, out_cap, out_len, status, count=None,
                       pool_len=None, stream=None) -> None:
    """MessageBuilder.allocateStruct, the StructBuilder writes and toBytes (message.zig:1643-2170,
    message/struct_builder.zig:332-989) over a batch: the ops are applied to every message, with
    values from the op-major columns (entry k * n + i of value / length / count, int64, is op k of
    message i; a slice is d_pool[value : value + length]). Message i is written at
    d_out[out_off[i]:] and out_len[i] is its framed length; d_out=None gives sizes only."""
    n = _units(out_len, status)
    nops = len(ops)
    _check_field_major((value, length, count), nops, n, "messages")
    if d_out is not None:
        _units(out_len, out_off, out_cap)  # out_off may be a lengths_to_offsets result (n + 1 entries)
    if pool_len is None:
        pool_len = 0 if d_pool is None else d_pool.numel() * d_pool.element_size()
    arr = (CBuildOp * max(1, nops))()  # read by the call itself (passed to the kernel by value)
    for i, o in enumerate(ops):
        arr[i] = o.c()
    _raise(lib().capnp_packed_build_fields_batch(_ptr(d_pool), int(pool_len), n, ctypes.addressof(arr), nops,
                                                 _ptr(value), _ptr(length), _ptr(count), _ptr(d_out),
                                                 _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status),
                                                 _stream(stream)), "build_fields_batch")


# capnp_packed_list_heads_batch / capnp_packed_read_elements_batch list kinds
LIST_STRUCT, LIST_POINTER = 0, 1


class CListHead(ctypes.Structure):
    """struct capnp_packed_list_head"""
    _fields_ = [("elems_off", ctypes.c_uint64), ("count", ctypes.c_uint32), ("segment", ctypes.c_uint32),
                ("seg_begin", ctypes.c_uint32), ("seg_bytes", ctypes.c_uint32), ("data_words", ctypes.c_uint16),
                ("pointer_words", ctypes.c_uint16), ("status", ctypes.c_int32)]


LIST_HEAD_DTYPE = np.dtype([("elems_off", "<u8"), ("count", "<u4"), ("segment", "<u4"), ("seg_begin", "<u4"),
                            ("seg_bytes", "<u4"), ("data_words", "<u2"), ("pointer_words", "<u2"),
                            ("status", "<i4")])
LIST_HEAD_BYTES = 32


def list_heads_batch(d_in, in_off, in_len, list_kind, pointer_index, head, count, status, path=(),
                     stream=None) -> None:
    """readStructList (LIST_STRUCT) or readTextList / readPointerList (LIST_POINTER) of pointer
    `pointer_index` of the struct at `path` from the root, one list per framed message: head
    (uint8, 32 bytes a message: CListHead / LIST_HEAD_DTYPE), count (int64) and status (int32)."""
    n = _units(in_off, in_len, count, status)
    _check_head(head, n)
    path = tuple(int(p) for p in path)
    arr = (ctypes.c_uint32 * max(1, len(path)))(*path)
    _raise(lib().capnp_packed_list_heads_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, ctypes.addressof(arr),
                                               len(path), pointer_index, list_kind, _ptr(head), _ptr(count),
                                               _ptr(status), _stream(stream)), "list_heads_batch")


def read_elements_batch(d_in, in_off, in_len, head, elem_start, list_kind, elem_cap, fields, value, length, status,
                        count=None, parent=None, index=None, stream=None) -> None:
    """Fields of every element of the lists `head` describes, as columns over the elements:
    entry f * elem_cap + e of value / length / count (int64) and status (int32) is field f of
    element e; parent / index (int32, optional) are the element's message and its place in that
    message's list. elem_start = lengths_to_offsets(counts)."""
    n = _units(in_off, in_len)
    nf = len(fields)
    elem_cap = int(elem_cap)
    if elem_start is not None and elem_start.numel() < n + 1:
        raise InvalidArgument(f"elem_start has {elem_start.numel()} entries for {n} messages")
    _check_head(head, n)
    _check_field_major((value, length, status, count), nf, elem_cap, "elements")
    for t in (parent, index):
        if t is not None and t.numel() < elem_cap:
            raise InvalidArgument(f"per-element output has {t.numel()} entries for {elem_cap} elements")
    arr = _cfields(fields)
    _raise(lib().capnp_packed_read_elements_batch(_ptr(d_in), _ptr(in_off), _ptr(in_len), n, _ptr(head),
                                                  _ptr(elem_start), list_kind, elem_cap, ctypes.addressof(arr), nf,
                                                  _ptr(parent), _ptr(index), _ptr(value), _ptr(length), _ptr(count),
                                                  _ptr(status), _stream(stream)), "read_elements_batch")


def read_list_batch(d_in, in_off, in_len, list_kind, pointer_index, fields, path=(), max_elements=None,
                    stream=None) -> tuple:
    """The whole chain: list_heads_batch -> lengths_to_offsets -> read_elements_batch. Returns
    (head_status, counts, start, total, parent, index, value, length, count, status); the four
    field outputs are [len(fields), capacity]. max_elements None: the total is read back (one
    sync) and the outputs are allocated exactly, total an int. A number: that capacity is
    allocated, nothing syncs and total is a device tensor (start[n:]) for the caller to compare:
    elements past the capacity were not read."""
    n = _units(in_off, in_len)
    dev = in_off.device
    head = torch.empty(n * LIST_HEAD_BYTES, dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int64, device=dev)
    head_status = torch.empty(n, dtype=torch.int32, device=dev)
    list_heads_batch(d_in, in_off, in_len, list_kind, pointer_index, head, counts, head_status, path, stream)
    start = lengths_to_offsets(counts, stream=stream)
    if max_elements is None:
        total = cap = int(start[n].item())
    else:
        cap = int(max_elements)
        total = start[n:]
    nf = len(fields)
    out = torch.zeros((3, nf, cap), dtype=torch.int64, device=dev)
    status = torch.zeros((nf, cap), dtype=torch.int32, device=dev)
    parent = torch.zeros(cap, dtype=torch.int32, device=dev)
    index = torch.zeros(cap, dtype=torch.int32, device=dev)
    read_elements_batch(d_in, in_off, in_len, head, start, list_kind, cap, fields, out[0], out[1], status,
                        out[2], parent, index, stream)
    return head_status, counts, start, total, parent, index, out[0], out[1], out[2], status


def lengths_to_offsets(lengths, base: int = 0, out=None, stream=None):
    """Exclusive scan of lengths -> n+1 offsets (dense output layout), on device."""
    n = lengths.numel()
    if out is None:
        out = torch.empty(n + 1, dtype=torch.int64, device=lengths.device)
    nbytes = lib().capnp_packed_scan_scratch_bytes(n)
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=lengths.device)
    _raise(lib().capnp_packed_lengths_to_offsets(_ptr(lengths), n, base, _ptr(out), _ptr(scratch), nbytes,
                                                 _stream(stream)), "lengths_to_offsets")
    return out


def generate(n_units: int, unit_bytes: int, seed: int, zero_thresh: int, unit_base: int = 0,
             out=None, device="cuda", stream=None):
    """Device-side synthetic units; twin of the oracle generator."""
    if out is None:
        out = torch.empty(n_units * unit_bytes, dtype=torch.uint8, device=device)
    _raise(lib().capnp_packed_generate(_ptr(out), n_units, unit_bytes, unit_base, seed, zero_thresh,
                                       _stream(stream)), "generate")
    return out


def uniform_layout(n_units: int, unit_bytes: int, device="cuda"):
    """(offsets, lengths) of n equal units laid out densely; also the capacity-slot
    layout of an encode output (unit_bytes = encode_bound(unit size))."""
    off = torch.arange(0, n_units * unit_bytes, unit_bytes, dtype=torch.int64, device=device)
    ln = torch.full((n_units,), unit_bytes, dtype=torch.int64, device=device)
    return off, ln
