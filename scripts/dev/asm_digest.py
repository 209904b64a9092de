#!/usr/bin/env python3
"""usage: asm_digest.py lib/packed_kernels.s  (from `make asm`)
One line per function symbol, sorted by name: NAME BODY_HASH DESCRIPTOR_HASH. The body runs from
`.type NAME,@function` to its `.size`; the descriptor is `.amdhsa_kernel .. .end_amdhsa_kernel`.
Left out of both: the symbol's own name, the function index in local labels (it follows the order
of definitions, also in comments) and runs of blanks (the comment column follows a label's width).
Equal digests = same ISA and resources. It only hashes."""
import hashlib
import re
import sys


def digest(lines, name):
    text = re.sub(r"(BB|func_begin|func_end|tmp|JTI|CPI)\d+", r"\1#", "".join(lines))
    text = re.sub(r"(?<![\w$.])%s(?![\w$.])" % re.escape(name), "@", text)
    return hashlib.sha256(re.sub(r"[ \t]+", " ", text).encode()).hexdigest()[:16]


parts, cur = {}, None  # (kind, name) -> lines
for line in open(sys.argv[1]):
    m = re.match(r"\s*\.(type|amdhsa_kernel)\s+([^\s,]+)(,@function)?\s*$", line)
    if m and (m.group(1) == "amdhsa_kernel" or m.group(3)):
        cur = parts.setdefault((m.group(1), m.group(2)), [])
    if cur is not None:
        cur.append(line)
        if re.match(r"\s*(\.size\s|\.end_amdhsa_kernel)", line):
            cur = None
for name in sorted(n for k, n in parts if k == "type"):
    desc = parts.get(("amdhsa_kernel", name))
    print(name, digest(parts[("type", name)], name), digest(desc, name) if desc else "-")
