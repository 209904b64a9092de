"""Model and generators for the framed-message encoders (capnp_packed_encode_framed_*;
DESIGN.md §2.12).

The model is plain Python: Message.init's segment-table parse (message.zig:341-394) plus the
rule that a unit is exactly its table and its segments, then the expected bytes from
pyref_cxx.pack_message (the C++ dialect) or the caller's whole-buffer packer (the Zig dialect).
Nothing here needs the GPU.
"""
import struct

import numpy as np

import pyref_cxx

OK = 0
INVALID_MESSAGE_SIZE = 1
OUT_OF_SPACE = 4
INVALID_ARGUMENT = 5
END_OF_STREAM = 8
INVALID_SEGMENT_COUNT = 9
SEGMENT_COUNT_LIMIT_EXCEEDED = 10
TRUNCATED_MESSAGE = 13

MAX_SEGS = 512
TILE_WORDS = 512          # the encoders' tile
MAX_WORDS = 0xFFFFF000    # word indices are u32


def message_init(unit: bytes):
    """Message.init: (status, segments). Trailing bytes are ignored, as the reference does."""
    n = len(unit)
    if n < 4:
        return END_OF_STREAM, None
    (m1,) = struct.unpack_from("<I", unit, 0)
    if m1 == 0xFFFFFFFF:
        return INVALID_SEGMENT_COUNT, None
    count = m1 + 1
    if count > MAX_SEGS:
        return SEGMENT_COUNT_LIMIT_EXCEEDED, None
    header = 4 * (1 + count + (0 if count & 1 else 1))
    if header > n:
        return TRUNCATED_MESSAGE, None
    sizes = struct.unpack_from(f"<{count}I", unit, 4)
    off = header
    segs = []
    for sw in sizes:
        end = off + 8 * sw
        if end > n:
            return TRUNCATED_MESSAGE, None
        segs.append(unit[off:end])
        off = end
    return OK, segs


def verdict(unit: bytes, address: int = 0):
    """The framed calls' per-unit checks in their order: (status, segments)."""
    if address % 8:
        return INVALID_ARGUMENT, None
    if len(unit) % 8:
        return INVALID_MESSAGE_SIZE, None
    st, segs = message_init(unit)
    if st != OK:
        return st, None
    used = 8 * ((1 + len(segs) + 1) // 2) + sum(len(s) for s in segs)
    if used < len(unit):
        return INVALID_ARGUMENT, None  # trailing words: the next message to a stream reader
    if len(unit) // 8 > MAX_WORDS:
        return INVALID_ARGUMENT, None
    return OK, segs


def expected(unit: bytes, dialect: str, zig_pack, address: int = 0):
    """(status, packed bytes) of one unit; zig_pack(bytes) -> bytes is packPacked."""
    st, segs = verdict(unit, address)
    if st != OK:
        return st, b""
    if dialect == "cxx":
        return OK, pyref_cxx.pack_message(segs)
    return OK, zig_pack(unit)


def route(unit: bytes, dialect: str, address: int = 0) -> str:
    """Which way the kernels code the unit: "fail", "tile" (one tile, one piece) or "walk"
    (piece by piece / tile by tile; in the dense call the two-pass route)."""
    st, segs = verdict(unit, address)
    if st != OK:
        return "fail"
    if len(unit) // 8 > TILE_WORDS:
        return "walk"
    return "walk" if dialect == "cxx" and len(segs) > 1 else "tile"


# ---------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------
def frame(segments, pad_word: int = 0) -> bytes:
    """toBytes: the segment table, then the segments (pad_word fills the padding half-word)."""
    segs = [bytes(s) for s in segments] or [b""]
    hdr = struct.pack("<I", len(segs) - 1) + b"".join(struct.pack("<I", len(s) // 8) for s in segs)
    if len(segs) % 2 == 0:
        hdr += struct.pack("<I", pad_word)
    return hdr + b"".join(segs)


def rand_words(rng, words: int, p: float) -> bytes:
    """words * 8 random bytes, each zero with probability p."""
    a = rng.integers(1, 256, 8 * words, dtype=np.uint8)
    a[rng.random(8 * words) < p] = 0
    return a.tobytes()


def class_words(rng, words: int) -> bytes:
    """Words drawn from the classes the C++ rule tells apart (Z, A, B, C), in short runs, so
    that runs end and start at piece boundaries often."""
    out = bytearray()
    k = int(rng.integers(0, 1000))
    while len(out) < 8 * words:
        kind = "ZABC"[int(rng.integers(0, 4))]
        for _ in range(int(rng.integers(1, 5))):
            out += {"Z": lambda _k: pyref_cxx.WORD_Z, "A": pyref_cxx.word_a, "B": pyref_cxx.word_b,
                    "C": pyref_cxx.word_c}[kind](k)
            k += 1
    return bytes(out[:8 * words])


def random_frame(rng, max_segs: int = 40, max_words: int = 3 * TILE_WORDS) -> bytes:
    """A valid framed message of 1 .. max_segs segments and at most max_words framed words."""
    count = int(rng.integers(1, max_segs + 1))
    hw = count // 2 + 1
    budget = int(rng.integers(0, max(1, max_words - hw)))
    cuts = np.sort(rng.integers(0, budget + 1, count - 1)) if count > 1 else np.array([], dtype=np.int64)
    sizes = np.diff(np.concatenate(([0], cuts, [budget]))).astype(int)
    segs = []
    for sw in sizes:
        segs.append(class_words(rng, int(sw)) if rng.random() < 0.5 else rand_words(rng, int(sw), float(rng.choice([0.02, 0.5, 0.9]))))
    return frame(segs)


def count_field(m1: int, nbytes: int = 8) -> bytes:
    """A unit of nbytes whose count field is m1 and whose other bytes are zero."""
    return struct.pack("<I", m1) + bytes(nbytes - 4)


def error_units():
    """name -> (unit, expected status): every per-unit error an aligned unit can have."""
    a = pyref_cxx.words
    return {
        "table_overruns_unit": (count_field(511, 8), TRUNCATED_MESSAGE),
        "segment_past_data": (frame([a("A*4")])[:-8], TRUNCATED_MESSAGE),
        "second_segment_past_data": (struct.pack("<IIII", 1, 1, 3, 0) + a("A*3"), TRUNCATED_MESSAGE),
        "one_trailing_word": (frame([a("A B")]) + bytes(8), INVALID_ARGUMENT),
        "trailing_after_three": (frame([a("A"), a("Z"), b""]) + a("A"), INVALID_ARGUMENT),
        "empty_unit": (b"", END_OF_STREAM),
        "len_4_mod_8": (frame([a("A*2")])[:-4], INVALID_MESSAGE_SIZE),
        "count_513": (count_field(512, 8 * 258), SEGMENT_COUNT_LIMIT_EXCEEDED),
        "count_ffffffff": (count_field(0xFFFFFFFF, 16), INVALID_SEGMENT_COUNT),
    }


def boundary_units():
    """name -> segments: the piece-boundary cases (runs that would cross a boundary if packing
    did not restart there)."""
    a = pyref_cxx.words
    return {
        "ZZ|ZZ": [a("Z Z"), a("Z Z")],
        "AA|AA": [a("A A"), a("A A")],
        "A|B": [a("A"), a("B")],
        "k,0,0": [a("Z*3 A"), b"", b""],
        "A*257": [a("A*257"), a("A")],
    }


def count_units(rng):
    """name -> unit for the segment counts the table check branches on (all OK)."""
    out = {}
    for c in (1, 2, 3, 63, 64, 65, 511, 512):
        out[f"count_{c}"] = frame([class_words(rng, int(rng.integers(0, 4))) for _ in range(c)])
    out["all_empty_7"] = frame([b""] * 7)
    out["all_empty_512"] = frame([b""] * 512)
    out["table_alone"] = frame([b""])
    return out


def tile_edge_units(rng):
    """name -> unit around the 512-word tile (all OK)."""
    out = {}
    for fw in (511, 512, 513):  # framed words of a single-segment unit
        out[f"single_{fw}"] = frame([rand_words(rng, fw - 1, 0.5)])
    for pw in (512, 513, 1025):  # a piece of that many words among others
        # two table words, then 3 words: the piece starts at word 5, at 8 mod 16 in a 16-aligned unit
        out[f"piece_{pw}_at8"] = frame([class_words(rng, 3), rand_words(rng, pw, 0.5)])
        # the piece starts at word 2, at 0 mod 16: its full tiles are read straight from memory
        out[f"piece_{pw}_at0"] = frame([rand_words(rng, pw, 0.5), class_words(rng, 5), b""])
    # odd table words: every first segment starts at 8 mod 16 (the unit itself 16-aligned)
    out["first_at_8_mod_16_a"] = frame([rand_words(rng, 512, 0.1), rand_words(rng, 7, 0.5)] + [b""] * 2)  # 4 segs: hw 3
    out["first_at_8_mod_16_b"] = frame([rand_words(rng, 600, 0.5)])                                       # 1 seg: hw 1
    return out
