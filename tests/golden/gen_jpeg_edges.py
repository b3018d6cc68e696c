"""Generates tests/golden/jpeg_edges/*.jpg and jpeg_edge_pins.json: small JPEGs at the edges of the decoder (tests/test_jpeg_edges.py) —
IDCT range limiting, tiny and odd sizes at every sampling, restart intervals in progressive scans, RGB-coded and EXIF-rotated
files — encoded with Pillow from seeded random arrays, and the pins = shape and SHA-256 of libjpeg-turbo's decode (Pillow's decoder,
the library family behind cv::imdecode) of every file and of every byte-surgery variant of tests/jpeg_surgery.py, or
"refuse": "<reason>" for the streams that must not be decoded.  gen_jpeg_fixtures.py and its files are not touched.
Run once: python tests/golden/gen_jpeg_edges.py"""
import hashlib, io, json, os, sys
import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_surgery

out = os.path.join(HERE, "jpeg_edges")
os.makedirs(out, exist_ok=True)
SAMPLINGS = {"444": 0, "422": 1, "420": 2}


def noise(seed, w, h):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def saturated(seed, w, h):
    return (np.random.RandomState(seed).randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


def patches(seed, w, h):
    """Flat 8x8 cells (end-of-band runs over several blocks), noise over the left half (blocks with every band filled)."""
    rs = np.random.RandomState(seed)
    a = np.repeat(np.repeat(rs.randint(0, 256, ((h + 7) // 8, (w + 7) // 8, 3)), 8, 0), 8, 1)[:h, :w].astype(np.int64)
    a[:, : w // 2] += rs.randint(-40, 41, (h, w // 2, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def exif(order, value):
    """Exif APP1 payload: a TIFF header and an IFD0 with the one tag 0x0112 (Orientation, SHORT, count 1)."""
    e = {"II": "little", "MM": "big"}[order]
    n = lambda v, k: v.to_bytes(k, e)
    return (b"Exif\0\0" + order.encode() + n(42, 2) + n(8, 4) + n(1, 2) + n(0x0112, 2) + n(3, 2) + n(1, 4) + n(value, 2) + n(0, 2) + n(0, 4))


files = {}      # name -> (array or PIL image, save options)
refuse = {}     # name -> reason

# ---- range limiting in the IDCT: 52x40 = 48 luma + 12 + 12 chroma blocks at 4:2:0, both component boundaries inside the second 32-block workgroup
for kind, make in (("noise", noise), ("sat", saturated)):
    for s, sub in SAMPLINGS.items():
        for q in (100, 5):
            for mode in ("base", "prog"):
                files["rng_%s_%s_q%d_%s.jpg" % (kind, s, q, mode)] = (make(11, 52, 40), dict(subsampling=sub, quality=q, progressive=mode == "prog"))
files["rng_noise_420_qt1.jpg"] = (noise(12, 52, 40), dict(subsampling=2, qtables=[[1] * 64, [1] * 64]))
files["rng_sat_420_qt255.jpg"] = (saturated(12, 52, 40), dict(subsampling=2, qtables=[[255] * 64, [255] * 64]))

# ---- sizes (width x height)
SIZES = [(1, 1), (2, 1), (1, 2), (2, 2), (4, 3), (5, 3), (17, 1), (1, 17), (8, 8), (16, 16), (15, 16), (16, 15), (17, 17), (65, 5), (130, 3), (1030, 9)]
for w, h in SIZES:
    for s, sub in SAMPLINGS.items():
        for mode in ("base",) if w == 1030 else ("base", "prog"):
            files["sz_%dx%d_%s_%s.jpg" % (w, h, s, mode)] = (noise(1000 * w + h, w, h), dict(subsampling=sub, quality=90 if w < 1030 else 60, progressive=mode == "prog"))

# ---- restart intervals: EOBRUN and predictor reset in the non-interleaved scans of a progressive frame
for s, sub in SAMPLINGS.items():
    for b in (1, 2, 5):
        files["rst_prog_%s_b%d.jpg" % (s, b)] = (patches(21, 47, 33), dict(subsampling=sub, progressive=True, restart_marker_blocks=b))
files["rst_prog_grey_b2.jpg"] = (Image.fromarray(patches(22, 47, 33)).convert("L"), dict(progressive=True, restart_marker_blocks=2))
files["rst_prog_422_rows2.jpg"] = (patches(23, 47, 33), dict(subsampling=1, progressive=True, restart_marker_rows=2))
files["rst_base_420_b1.jpg"] = (patches(24, 47, 33), dict(subsampling=2, restart_marker_blocks=1))

# ---- streams that libjpeg-turbo / imdecode read differently from a plain YCbCr decode: refused
files["rgb_444.jpg"] = (noise(31, 17, 9), dict(subsampling=0, quality=90, keep_rgb=True))
refuse["rgb_444.jpg"] = "RGB-coded JPEG"
for o in range(1, 9):
    files["exif_o%d.jpg" % o] = (noise(32, 19, 11), dict(subsampling=2, quality=90, exif=exif("II" if o % 2 else "MM", o)))
    if o > 1:
        refuse["exif_o%d.jpg" % o] = "EXIF orientation %d" % o

for name, (im, kw) in files.items():
    im = im if isinstance(im, Image.Image) else Image.fromarray(im)
    bio = io.BytesIO()
    im.save(bio, "JPEG", **kw)
    open(os.path.join(out, name), "wb").write(bio.getvalue())
# one committed file with fill bytes in front of its restart markers (the sanitizer program of tests/test_host_sanitizers.py reads files)
files["rst_base_420_b1_fill.jpg"] = None
open(os.path.join(out, "rst_base_420_b1_fill.jpg"), "wb").write(jpeg_surgery.variant(out, "rst_base_420_b1.jpg#fill_rst"))


def pin(data):
    rgb = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return {"shape": list(rgb.shape), "sha256": hashlib.sha256(rgb.tobytes()).hexdigest()}


refuse.update(jpeg_surgery.VARIANT_REFUSALS)
pins = {"_decoder": "Pillow %s / libjpeg-turbo %s (jpeglib %s)" % (Image.__version__, features.version("libjpeg_turbo"), features.version("jpg"))}
for key in list(files) + ["%s#%s" % v for v in jpeg_surgery.VARIANTS]:
    data = jpeg_surgery.variant(out, key)
    pins[key] = {"refuse": refuse[key]} if key in refuse else pin(data)
sizes = [os.path.getsize(os.path.join(out, n)) for n in files]
assert max(sizes) <= 16 << 10 and sum(sizes) < 300 << 10, (max(sizes), sum(sizes))
json.dump(pins, open(os.path.join(HERE, "jpeg_edge_pins.json"), "w"), indent=1, sort_keys=True)
print(len(pins) - 1, "pins written;", len(files), "files,", sum(sizes), "bytes, largest", max(sizes))
