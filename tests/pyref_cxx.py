"""Plain Python / numpy restatement of the C++-canonical packing rule.

Written from the rule's statement, not from any C++ source. Words are 8 bytes: Z is all
zero, A has no zero byte, B exactly one, C two to seven.
  Z:      00, then the number of immediately following Z words (at most 255), which are skipped.
  A:      FF, the word's 8 bytes, then the number r of immediately following A-or-B words (at
          most 255), then those r words raw.
  B or C: the tag (bit k set <=> byte k non-zero), then the non-zero bytes in order.
Packing restarts at every piece: a raw buffer is one piece; a message's pieces are its
segment table (8 * ceil((1 + nseg) / 2) bytes) and then each segment.
"""
import struct

import numpy as np


def _zero_bytes_per_word(data: bytes) -> np.ndarray:
    a = np.frombuffer(data, dtype=np.uint8).reshape(-1, 8)
    return (a == 0).sum(axis=1)


def pack_piece(data) -> bytes:
    data = bytes(data)
    if len(data) % 8:
        raise ValueError("piece length is not a multiple of 8")
    n = len(data) // 8
    if n == 0:
        return b""
    nz = _zero_bytes_per_word(data).tolist()
    out = bytearray()
    i = 0
    while i < n:
        w = data[8 * i:8 * i + 8]
        if nz[i] == 8:
            r = 0
            while r < 255 and i + 1 + r < n and nz[i + 1 + r] == 8:
                r += 1
            out += bytes((0x00, r))
            i += 1 + r
        elif nz[i] == 0:
            r = 0
            while r < 255 and i + 1 + r < n and nz[i + 1 + r] <= 1:
                r += 1
            out += b"\xff" + w + bytes((r,)) + data[8 * (i + 1):8 * (i + 1 + r)]
            i += 1 + r
        else:
            out.append(sum(1 << k for k in range(8) if w[k]))
            out += w.translate(None, b"\x00")  # the non-zero bytes, in order
            i += 1
    return bytes(out)


def pack_buffer(data) -> bytes:
    """A raw buffer is one piece."""
    return pack_piece(data)


def segment_table(segments) -> bytes:
    segs = list(segments) or [b""]
    hdr = struct.pack("<I", len(segs) - 1) + b"".join(struct.pack("<I", len(s) // 8) for s in segs)
    if len(segs) % 2 == 0:
        hdr += bytes(4)
    assert len(hdr) == 8 * ((1 + len(segs) + 1) // 2)
    return hdr


def pack_message(segments) -> bytes:
    """The segment table and then each segment, every piece packed on its own."""
    segs = [bytes(s) for s in segments] or [b""]
    return pack_piece(segment_table(segs)) + b"".join(pack_piece(s) for s in segs)


def split_framed(framed: bytes):
    """The segments of a framed message (segment table + segments)."""
    (m1,) = struct.unpack_from("<I", framed, 0)
    count = m1 + 1
    sizes = struct.unpack_from(f"<{count}I", framed, 4)
    off = 8 * ((1 + count + 1) // 2)
    segs = []
    for sw in sizes:
        segs.append(framed[off:off + 8 * sw])
        off += 8 * sw
    return segs


# word makers for the tests
def word_a(k: int) -> bytes:
    return bytes(1 + (k + j) % 255 for j in range(8))


def word_b(k: int) -> bytes:
    w = bytearray(word_a(k))
    w[k % 8] = 0
    return bytes(w)


def word_c(k: int) -> bytes:  # six non-zero bytes
    w = bytearray(word_a(k))
    w[k % 8] = 0
    w[(k + 3) % 8] = 0
    return bytes(w)


WORD_Z = bytes(8)


def words(spec: str) -> bytes:
    """'A*256 B A' -> bytes; tokens A, B, C, Z with an optional *count."""
    out = bytearray()
    k = 0
    for tok in spec.split():
        name, _, cnt = tok.partition("*")
        for _ in range(int(cnt) if cnt else 1):
            out += {"A": word_a, "B": word_b, "C": word_c, "Z": lambda _k: WORD_Z}[name](k)
            k += 1
    return bytes(out)
