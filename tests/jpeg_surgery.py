"""Deterministic byte surgery on JPEG streams: legal variants of a committed fixture (ITU-T T.81 B.1.1.2: any marker may be preceded by
fill bytes FF; B.2.4.1: Pq = 1 tables; SOF1) that an encoder hardly ever writes.  Used by tests/golden/gen_jpeg_edges.py, which pins
libjpeg-turbo's decode of every variant, and by tests/test_jpeg_edges.py, which makes the same variants again at run time."""


def walk(data):
    """[(offset, marker, end)] of every marker of the stream, restart markers and the markers behind entropy-coded data included.
    end = the first byte behind the segment (behind the two marker bytes for RSTn / EOI)."""
    out = []
    i = 2
    while i + 1 < len(data):
        if data[i] != 0xFF or data[i + 1] in (0x00, 0xFF):
            i += 1                                   # entropy-coded data, a stuffed zero, a fill byte
            continue
        m = data[i + 1]
        if 0xD0 <= m <= 0xD9:
            out.append((i, m, i + 2))
            i += 2
            continue
        end = i + 2 + int.from_bytes(data[i + 2: i + 4], "big")
        out.append((i, m, end))
        i = end
    return out


def _insert(data, at):
    """at: {offset: bytes to put in front of that offset}"""
    out, last = [], 0
    for off in sorted(at):
        out += [data[last:off], at[off]]
        last = off
    return b"".join(out + [data[last:]])


def sof1(data):
    (off,) = [o for o, m, _ in walk(data) if m == 0xC0]
    return data[: off + 1] + b"\xc1" + data[off + 2:]


def dqt16(data, mul):
    """Every DQT rewritten with Pq = 1 (16-bit entries), the values times `mul`."""
    out, last = [], 0
    for off, m, end in walk(data):
        if m != 0xDB:
            continue
        body, new, k = data[off + 4: end], b"", 0
        while k < len(body):
            assert body[k] >> 4 == 0
            new += bytes([0x10 | body[k]]) + b"".join((v * mul).to_bytes(2, "big") for v in body[k + 1: k + 65])
            k += 65
        out += [data[last:off], b"\xff\xdb" + (len(new) + 2).to_bytes(2, "big") + new]
        last = end
    return b"".join(out + [data[last:]])


def fill(data, which):
    """1, 2, 3, 1, ... fill bytes in front of the markers `which(marker, index, after_first_sos)` picks."""
    at, sos_seen, n = {}, False, 0
    for k, (off, m, _) in enumerate(walk(data)):
        if which(m, k, sos_seen):
            at[off] = b"\xff" * (1 + n % 3)
            n += 1
        sos_seen |= m == 0xDA
    assert at
    return _insert(data, at)


def fill_rst(data):
    return fill(data, lambda m, k, s: 0xD0 <= m <= 0xD7)


def fill_eoi(data):
    return fill(data, lambda m, k, s: m == 0xD9)


def fill_sos(data):
    return fill(data, lambda m, k, s: m == 0xDA)


def fill_dht_between_scans(data):
    return fill(data, lambda m, k, s: m == 0xC4 and s)


def com_app7(data):
    """A comment and an APP7 segment of the largest length a segment can have, in front of the frame header."""
    (off,) = [o for o, m, _ in walk(data) if m in (0xC0, 0xC1, 0xC2)]
    com = b"edge fixture"
    app7 = bytes((7 * i + 3) & 255 for i in range(65533))
    return _insert(data, {off: b"\xff\xfe" + (len(com) + 2).to_bytes(2, "big") + com + b"\xff\xe7\xff\xff" + app7})


def dri0(data):
    off = [o for o, m, _ in walk(data) if m == 0xDA][0]
    return _insert(data, {off: b"\xff\xdd\x00\x04\x00\x00"})


def _segment(data, marker):
    return [(o, e) for o, m, e in walk(data) if m == marker][0]


def _patch_app1(data, at, new):
    """Bytes of the first APP1's payload replaced from payload offset `at` (Exif\\0\\0 = 0..5, TIFF header 6..13, IFD0 count 14..15,
    its first entry: tag 16..17, type 18..19, count 20..23, value 24..27)."""
    o, _ = _segment(data, 0xE1)
    return data[: o + 4 + at] + new + data[o + 4 + at + len(new):]


def exif_behind_sof(data):
    """The Exif segment moved between the frame header and the scan: the headers-only call cannot see it, the decode call must."""
    o, e = _segment(data, 0xE1)
    app1, rest = data[o:e], data[:o] + data[e:]
    return _insert(rest, {_segment(rest, 0xC0)[1]: app1})


def exif_cut(data):
    """The segment ends inside the IFD entry: nothing may be read behind it."""
    o, e = _segment(data, 0xE1)
    body = data[o + 4: o + 4 + 22]
    return data[:o] + b"\xff\xe1" + (len(body) + 2).to_bytes(2, "big") + body + data[e:]


def exif_second(data):
    """An Exif segment with orientation 1 (big-endian TIFF) in front of the file's own: the first one counts."""
    o, _ = _segment(data, 0xE1)
    body = b"Exif\0\0MM\x00\x2a\x00\x00\x00\x08\x00\x01\x01\x12\x00\x03\x00\x00\x00\x01\x00\x01\x00\x00\x00\x00\x00\x00"
    return _insert(data, {o: b"\xff\xe1" + (len(body) + 2).to_bytes(2, "big") + body})


def adobe_strip(data):
    """No APP14 any more: libjpeg decides by the component ids, which are R, G, B."""
    o, e = _segment(data, 0xEE)
    return data[:o] + data[e:]


def adobe_transform1(data):
    o, _ = _segment(data, 0xEE)
    return data[: o + 4 + 11] + b"\x01" + data[o + 4 + 12:]


def jfif_first(data):
    """A JFIF APP0 in front of the Adobe segment: JFIF means YCbCr whatever follows."""
    return _insert(data, {2: bytes.fromhex("ffe000104a46494600010100000100010000")})


SURGERY = {
    "exif_behind_sof": exif_behind_sof,
    "exif_cut": exif_cut,
    "exif_second": exif_second,
    "exif_magic43": lambda d: _patch_app1(d, 8, b"\x00\x2b"),          # (exif_o6.jpg is big-endian)
    "exif_type_long": lambda d: _patch_app1(d, 18, b"\x00\x04"),
    "exif_count2": lambda d: _patch_app1(d, 20, b"\x00\x00\x00\x02"),
    "exif_value9": lambda d: _patch_app1(d, 24, b"\x00\x09"),
    "exif_value0": lambda d: _patch_app1(d, 24, b"\x00\x00"),
    "exif_ifd_far": lambda d: _patch_app1(d, 10, b"\x7f\xff\xff\xf0"),   # IFD0 offset far outside the segment
    "adobe_strip": adobe_strip,
    "adobe_transform1": adobe_transform1,
    "jfif_first": jfif_first,
    "sof1": sof1,
    "dqt16": lambda d: dqt16(d, 1),
    "dqt16x3": lambda d: dqt16(d, 3),
    "fill_rst": fill_rst,
    "fill_eoi": fill_eoi,
    "fill_sos": fill_sos,
    "fill_dht": fill_dht_between_scans,
    "com_app7": com_app7,
    "dri0": dri0,
}

# (committed fixture under tests/golden/jpeg_edges, surgery): the pins' keys are "<fixture>#<surgery>"
VARIANTS = [
    ("rst_base_420_b1.jpg", "sof1"),
    ("rst_base_420_b1.jpg", "dqt16"),
    ("rst_base_420_b1.jpg", "dqt16x3"),
    ("rst_prog_420_b2.jpg", "dqt16"),
    ("rst_prog_420_b2.jpg", "dqt16x3"),
    ("rst_base_420_b1.jpg", "fill_rst"),
    ("rst_prog_420_b2.jpg", "fill_rst"),
    ("rst_prog_444_b1.jpg", "fill_rst"),
    ("rst_prog_422_rows2.jpg", "fill_rst"),
    ("rst_prog_grey_b2.jpg", "fill_rst"),
    ("rst_base_420_b1.jpg", "fill_eoi"),
    ("rst_prog_420_b2.jpg", "fill_eoi"),
    ("rst_base_420_b1.jpg", "fill_sos"),
    ("rst_prog_420_b2.jpg", "fill_sos"),
    ("rst_prog_420_b2.jpg", "fill_dht"),
    ("sz_17x17_420_base.jpg", "com_app7"),
    ("sz_17x17_420_prog.jpg", "com_app7"),
    ("sz_17x17_420_base.jpg", "dri0"),
    ("sz_17x17_420_prog.jpg", "dri0"),
    # the edges of the two refusal rules: what still decodes (libjpeg-turbo's picture is the pin), what is refused by the decode call alone
    ("exif_o6.jpg", "exif_behind_sof"),
    ("exif_o6.jpg", "exif_cut"),
    ("exif_o6.jpg", "exif_second"),
    ("exif_o6.jpg", "exif_magic43"),
    ("exif_o6.jpg", "exif_type_long"),
    ("exif_o6.jpg", "exif_count2"),
    ("exif_o6.jpg", "exif_value9"),
    ("exif_o6.jpg", "exif_value0"),
    ("exif_o6.jpg", "exif_ifd_far"),
    ("rgb_444.jpg", "adobe_strip"),
    ("rgb_444.jpg", "adobe_transform1"),
    ("rgb_444.jpg", "jfif_first"),
]
VARIANT_REFUSALS = {"exif_o6.jpg#exif_behind_sof": "EXIF orientation 6", "rgb_444.jpg#adobe_strip": "RGB-coded JPEG"}


def variant(golden_edges_dir, key):
    import os
    name, _, how = key.partition("#")
    data = open(os.path.join(golden_edges_dir, name), "rb").read()
    return SURGERY[how](data) if how else data
