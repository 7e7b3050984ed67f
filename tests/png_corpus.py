"""The PNG corpus of the device-decode tests (tests/test_png_device_host.py, tests/test_gpu_png_decode.py): about 60 small files
built in a few hundred milliseconds with Pillow and Python's zlib, every one with the pixels Pillow reads back from it.

1. Pillow-written files: RGB and L at compress_level 0, 1, 6, 9 (Pillow picks filters 1, 2 and 4 adaptively).
2. Files from the writer below: every row set to each of the filters 0-4 in turn plus a row-by-row mix, the stream made with the
   default strategy, Z_FIXED (BTYPE 1), Z_RLE, Z_HUFFMAN_ONLY, level 0 (stored blocks) and two Z_FULL_FLUSH points (several
   blocks), the IDAT data split into chunks of 1, 7 and 8192 bytes.
3. Sizes: widths 1, 2, 3, 32, 33; heights 1, 2, 32, 256, 416 (T = 13); one image of more than 65 535 raw bytes at level 0
   (several stored blocks).
4. Content: smooth plus noise; all-zero (long runs: length 258, distance 1, a single distance code); a block repeated at a
   distance between 16 385 and 32 768."""
import io
import struct
import zlib
from functools import lru_cache

import numpy as np

GUARD = 32


def image(w, h, c, seed=0, noise=12):
    """smooth plus noise, uint8 [h, w, c] ([h, w] for c = 1)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 120 + 60 * np.sin(x / 5.0 + seed) + 50 * np.cos(y / 9.0)
    a = base[..., None] + np.arange(c) * 9 + rng.integers(-noise, noise + 1, (h, w, c))
    a = np.clip(a, 1, 255).astype(np.uint8)
    return a if c > 1 else a[..., 0]


def _paeth(a, b, c):
    p = a.astype(np.int16) + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c)).astype(np.uint8)


def filter_rows(img, filters):
    """raw scanlines of `img` with row r filtered by type filters[r % len(filters)]"""
    h, w = img.shape[:2]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    rows = img.reshape(h, w * bpp).astype(np.uint8)
    out = bytearray()
    zero = np.zeros(w * bpp, np.uint8)
    for r in range(h):
        f = filters[r % len(filters)]
        cur, up = rows[r], rows[r - 1] if r else zero
        left = np.concatenate([np.zeros(bpp, np.uint8), cur[:-bpp]]) if w * bpp > bpp else np.zeros(w * bpp, np.uint8)
        upleft = np.concatenate([np.zeros(bpp, np.uint8), up[:-bpp]]) if w * bpp > bpp else np.zeros(w * bpp, np.uint8)
        pred = {0: zero, 1: left, 2: up, 3: ((left.astype(np.uint16) + up) >> 1).astype(np.uint8), 4: _paeth(left, up, upleft)}[f]
        out.append(f)
        out += (cur - pred).astype(np.uint8).tobytes()
    return bytes(out)


def deflate(raw, how):
    if how == "default":
        return zlib.compress(raw, 6)
    if how == "best":
        return zlib.compress(raw, 9)
    if how == "level0":
        return zlib.compress(raw, 0)
    if how == "flush":
        co = zlib.compressobj(6)
        a, b = len(raw) // 3, 2 * len(raw) // 3
        return co.compress(raw[:a]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(raw[a:b]) + co.flush(zlib.Z_FULL_FLUSH) + \
            co.compress(raw[b:]) + co.flush()
    strategy = {"fixed": zlib.Z_FIXED, "rle": zlib.Z_RLE, "huffman": zlib.Z_HUFFMAN_ONLY}[how]
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
    return co.compress(raw) + co.flush()


def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)


def container(w, h, ctype, stream, split=1 << 30, depth=8, interlace=0, extra=b""):
    idat = b"".join(_chunk(b"IDAT", stream[k:k + split]) for k in range(0, len(stream), split))
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace)) + extra + idat + \
        _chunk(b"IEND", b"")


def write_png(img, filters, how, split=1 << 30):
    h, w = img.shape[:2]
    return container(w, h, 2 if img.ndim == 3 else 0, deflate(filter_rows(img, filters), how), split)


def pillow_png(img, **kw):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "PNG", **kw)
    return f.getvalue()


def pillow_pixels(data):
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)))


@lru_cache(maxsize=None)
def corpus():
    """[(name, file bytes, pixels as Pillow reads them)], built once per process"""
    files = []
    for c, mode in ((3, "rgb"), (1, "l")):                                   # 1. Pillow's writer
        for level in (0, 1, 6, 9):
            files.append((f"pillow_{mode}_l{level}", pillow_png(image(32, 64, c, seed=level), compress_level=level)))
    splits = (1, 7, 8192)
    k = 0
    for fi, filters in enumerate(((0,), (1,), (2,), (3,), (4,), (4, 0, 3, 1, 2, 2, 4, 1))):     # 2. our writer
        for how in ("default", "fixed", "rle", "huffman", "level0", "flush"):
            img = image(33 if k % 2 else 32, 32, 1 if k % 5 == 4 else 3, seed=100 + k)
            files.append((f"own_f{fi}_{how}_s{splits[k % 3]}", write_png(img, filters, how, splits[k % 3])))
            k += 1
    for n, (w, h) in enumerate(((1, 1), (2, 2), (3, 32), (32, 256), (33, 416), (1, 416), (2, 256), (3, 1), (32, 2), (33, 1),
                                (32, 416))):                                  # 3. sizes
        c = 1 if n % 3 == 2 else 3
        files.append((f"size_{w}x{h}_c{c}", pillow_png(image(w, h, c, seed=200 + n)) if n % 2 else
                      write_png(image(w, h, c, seed=200 + n), (4, 3, 1, 2, 0), "default", 8192)))
    big = image(160, 160, 3, seed=300)                                        # 76 960 raw bytes: two stored blocks
    files.append(("stored_multi", write_png(big, (0,), "level0", 8192)))
    zeros = np.zeros((416, 32, 3), np.uint8)                                  # 4. content
    files.append(("zeros_default", write_png(zeros, (0,), "best")))
    files.append(("zeros_rle", write_png(zeros, (2,), "rle", 7)))
    files.append(("zeros_pillow", pillow_png(zeros)))
    block = np.random.default_rng(7).integers(1, 256, (128, 64, 3), dtype=np.uint8)       # 128 x 193 = 24 704 raw bytes, twice
    files.append(("far_repeat", write_png(np.concatenate([block, block]), (0,), "best", 8192)))
    return [(name, data, pillow_pixels(data)) for name, data in files]


def refused_files():
    """{reason: file bytes} of legal PNGs the device decoder hands back to the host reader"""
    from PIL import Image
    rgb = image(8, 8, 3, seed=1)
    out = {}
    f = io.BytesIO()
    Image.fromarray(rgb).convert("P").save(f, "PNG")
    out["palette"] = f.getvalue()
    out["alpha"] = pillow_png(np.dstack([rgb, rgb[..., :1]]))
    f = io.BytesIO()
    Image.fromarray(rgb).convert("LA").save(f, "PNG")
    out["alpha_la"] = f.getvalue()
    out["16-bit"] = pillow_png((image(8, 8, 1, seed=2).astype(np.uint16) * 257))
    raw = filter_rows(rgb, (0,))
    out["interlaced"] = container(8, 8, 2, zlib.compress(raw), interlace=1)       # the container only: parse_png reads no pixels
    return out


def malformed_image():
    return image(14, 8, 3, seed=5, noise=6)


def malformed_streams():
    """(w, h, c, the good stream of about 300 bytes, [damaged copies]): a truncation at every byte and every single-bit flip of the
    first 64 bytes"""
    img = malformed_image()
    h, w, c = img.shape
    good = zlib.compress(filter_rows(img, (4, 1, 2, 3, 0)), 9)
    assert 250 <= len(good) <= 350 and (good[2] >> 1) & 3 == 2, len(good)      # one dynamic block: the flips reach its code lengths
    bad = [good[:n] for n in range(len(good))]
    for byte in range(64):
        for bit in range(8):
            b = bytearray(good)
            b[byte] ^= 1 << bit
            bad.append(bytes(b))
    return w, h, c, good, bad


def named_malformed():
    """three damaged streams with known causes, for the mixed GPU launch: (w, h, c, {name: stream})"""
    w, h, c = 16, 8, 3
    raw = filter_rows(image(w, h, c, seed=6), (0,))
    good = zlib.compress(raw, 6)
    stored = bytearray(zlib.compress(raw, 0))
    stored[5] ^= 0xff                                  # NLEN of the first stored block (2 header bytes, 1 block byte, LEN, NLEN)
    # a fixed-code block whose first symbol is a match: length 3 (symbol 257 = 0000001), distance code 0 (00000) -> distance 1 at position 0
    far = bytes([0x78, 0x9c]) + bytes([0b00000011, 0b00000010, 0, 0, 0, 0, 0, 0])
    return w, h, c, {"truncated": good[:len(good) // 2], "stored_nlen": bytes(stored), "too_far": far}
