"""Writer of small binary USD ("crate") files for the reader's tests: a scene's hydrodynamics table (the shape
`usd_crate.hydrodynamics_table` returns) back into a file that reader decodes - TOKENS / FIELDS / FIELDSETS / PATHS /
SPECS sections, LZ4 blocks (literals only) in TfFastCompression framing, USD's 2-bit-code integer compression, inlined
float / int / token values and out-of-line double 3-vectors.  Attributes the reader must pass over (an array value, a
token value, a prim that carries no hydrodynamics parameters) are written beside the table's own."""
from __future__ import annotations

import struct

from silver2_isaacsim_amd import config as cfg
from silver2_isaacsim_amd import usd_crate as uc

PREFIX = f"{cfg.EXPOSED_ATTR_NS}:{cfg.BEHAVIOR_NS}:"
SCENE_PRIM = "/World/PhysicsScene"


def lz4_literals(data: bytes) -> bytes:
    """One TfFastCompression chunk (leading 0) holding one LZ4 block of literals only."""
    n, ext = len(data), b""
    if n >= 15:
        rest = n - 15
        ext = b"\xff" * (rest // 255) + bytes([rest % 255])
    return b"\x00" + bytes([min(n, 15) << 4]) + ext + data


def encode_ints(values) -> bytes:
    """USD integer compression of 32-bit values (running sums of deltas), the inverse of usd_crate.decode_ints."""
    deltas, prev = [], 0
    for v in values:
        d = (v - prev) & 0xFFFFFFFF
        deltas.append(d - (1 << 32) if d & 0x80000000 else d)
        prev = v & 0xFFFFFFFF
    common = max(set(deltas), key=deltas.count) if deltas else 0
    codes, tail = bytearray((len(deltas) * 2 + 7) // 8), b""
    for i, d in enumerate(deltas):
        if d == common:
            code = 0
        elif -128 <= d < 128:
            code, tail = 1, tail + struct.pack("<b", d)
        elif -32768 <= d < 32768:
            code, tail = 2, tail + struct.pack("<h", d)
        else:
            code, tail = 3, tail + struct.pack("<i", d)
        codes[i >> 2] |= code << ((i & 3) * 2)
    return struct.pack("<i", common) + bytes(codes) + tail


def _compressed_ints(values) -> bytes:
    blob = lz4_literals(encode_ints(values))
    return struct.pack("<Q", len(blob)) + blob


def _rep(t: int, payload: int, flags: int = 0) -> int:
    return flags | (t << 48) | (payload & ((1 << 48) - 1))


class _Tree:
    """Prim / property paths in the crate's pre-order encoding (jump > 0: child at i + 1 and sibling at i + jump;
    -1: child only; 0: sibling only, at i + 1; -2: neither)."""

    def __init__(self):
        self.children: dict[str, list[str]] = {"/": []}

    def add(self, path: str):
        prim, _, prop = path.partition(".")
        parts = [p for p in prim.split("/") if p]
        parent = "/"
        for k in range(len(parts)):
            node = "/" + "/".join(parts[:k + 1])
            if node not in self.children:
                self.children[node] = []
                self.children[parent].append(node)
            parent = node
        if prop:
            self.children[path] = []
            self.children[parent].append(path)

    def encode(self, token):
        order = []                                  # (path, element token, jump)

        def walk(path, has_sibling):
            i = len(order)
            order.append(None)
            kids = self.children[path]
            for k, c in enumerate(kids):
                walk(c, k + 1 < len(kids))
            name = path.rsplit(".", 1)[1] if "." in path else path.rsplit("/", 1)[1]
            tok = 0 if path == "/" else (-token(name) if "." in path else token(name))
            if kids and has_sibling:
                jump = len(order) - i
            else:
                jump = -1 if kids else (0 if has_sibling else -2)
            order[i] = (path, tok, jump)
        walk("/", False)
        return order


def write_crate(path: str, table: dict) -> str:
    """A crate file whose `usd_crate.hydrodynamics_table` is `table` (floats that are fp32 values, as the scenes store them)."""
    tokens = [""]                                   # token 0 is never an element name: a property's token is stored negated

    def token(s: str) -> int:
        if s not in tokens:
            tokens.append(s)
        return tokens.index(s)

    out_of_line = bytearray()
    base = 24                                       # the value blob starts right after the header

    def vec3d(v) -> int:
        off = base + len(out_of_line)
        out_of_line.extend(struct.pack("<3d", *v))
        return _rep(uc._T_VEC3D, off)

    def f32(x) -> int:
        return _rep(uc._T_FLOAT, struct.unpack("<I", struct.pack("<f", x))[0], uc._INLINED)

    attrs: list[tuple[str, int]] = []               # (attribute path, value rep of `default`)
    for prim, entry in table.items():
        if prim == "__scene__":
            continue
        for name, val in entry.items():
            if name == "mass":
                attrs.append((f"{prim}.physics:mass", f32(val)))
            elif name == "translate":
                attrs.append((f"{prim}.xformOp:translate", vec3d(val)))
            else:
                attrs.append((f"{prim}.{PREFIX}{name}", f32(val)))
        attrs.append((f"{prim}.points", _rep(uc._T_VEC3F, 0, uc._ARRAY)))               # an array value: passed over
    attrs.append(("/World/GroundPlane.physics:mass", f32(1000.0)))                      # no hydrodynamics parameters: not in the table
    attrs.append(("/World/GroundPlane.xformOp:translate", vec3d((0.0, 0.0, -50.0))))
    attrs.append(("/World/GroundPlane.purpose", _rep(uc._T_TOKEN, token("default"), uc._INLINED)))
    if "timeStepsPerSecond" in table.get("__scene__", {}):
        attrs.append((f"{SCENE_PRIM}.physxScene:timeStepsPerSecond", _rep(uc._T_INT, table["__scene__"]["timeStepsPerSecond"], uc._INLINED)))

    tree = _Tree()
    for p, _ in attrs:
        tree.add(p)
    encoded = tree.encode(token)
    paths = [p for p, _, _ in encoded]

    fields: list[tuple[int, int]] = []              # (token of the field name, value rep)
    fieldsets: list[int] = []
    spec_rows = []                                  # (path index, fieldset index, spec type)
    rep_of = dict(attrs)
    for i, p in enumerate(paths):
        start = len(fieldsets)
        if p in rep_of:
            fields.append((token("typeName"), _rep(uc._T_TOKEN, token("float"), uc._INLINED)))
            fieldsets.append(len(fields) - 1)
            fields.append((token("default"), rep_of[p]))
            fieldsets.append(len(fields) - 1)
            kind = 1                                # attribute
        else:
            fields.append((token("specifier"), _rep(uc._T_TOKEN, token("def"), uc._INLINED)))
            fieldsets.append(len(fields) - 1)
            kind = 6                                # prim
        fieldsets.append(0xFFFFFFFF)
        spec_rows.append((i, start, kind))

    sections = {}
    raw = b"".join(t.encode() + b"\0" for t in tokens)
    blob = lz4_literals(raw)
    sections["TOKENS"] = struct.pack("<QQQ", len(tokens), len(raw), len(blob)) + blob
    reps = lz4_literals(struct.pack(f"<{len(fields)}Q", *[r for _, r in fields]))
    sections["FIELDS"] = (struct.pack("<Q", len(fields)) + _compressed_ints([t for t, _ in fields])
                          + struct.pack("<Q", len(reps)) + reps)
    sections["FIELDSETS"] = struct.pack("<Q", len(fieldsets)) + _compressed_ints(fieldsets)
    sections["PATHS"] = (struct.pack("<QQ", len(paths), len(encoded)) + _compressed_ints(range(len(encoded)))
                         + _compressed_ints([t & 0xFFFFFFFF for _, t, _ in encoded])
                         + _compressed_ints([j & 0xFFFFFFFF for _, _, j in encoded]))
    sections["SPECS"] = (struct.pack("<Q", len(spec_rows)) + _compressed_ints([r[0] for r in spec_rows])
                         + _compressed_ints([r[1] for r in spec_rows]) + _compressed_ints([r[2] for r in spec_rows]))

    body, toc = bytearray(out_of_line), []
    for name, data in sections.items():
        toc.append((name, base + len(body), len(data)))
        body.extend(data)
    toc_off = base + len(body)
    head = b"PXR-USDC" + bytes([0, 8, 0, 0, 0, 0, 0, 0]) + struct.pack("<q", toc_off)
    tail = struct.pack("<Q", len(toc)) + b"".join(n.encode().ljust(16, b"\0") + struct.pack("<qq", s, z) for n, s, z in toc)
    with open(path, "wb") as f:
        f.write(head + bytes(body) + tail)
    return path
