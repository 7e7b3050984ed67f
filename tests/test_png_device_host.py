"""CPU: the PNG container parser and the decoder core of `png_decode: device` through its host twin (ssr_png_decode_host: the text of
csrc/png_inflate.h that the kernel compiles, built for the host).  Every comparison is exact byte equality - with Pillow for
files, with zlib.decompress for streams."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_corpus as PC
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from satlas_super_resolution_amd import hip
    return hip.lib()


def _guards_intact(dst, offs, sizes, guard):
    """every byte of dst outside the images' ranges is still 0xA5"""
    mask = np.ones(dst.shape, bool)
    for o, n in zip(offs, sizes):
        mask[o:o + n] = False
        pad = (n + 15) // 16 * 16
        assert (dst[o + n:o + pad + guard] == 0xA5).all()
    return bool((dst[mask] == 0xA5).all())


def test_parse_png_accepts_gray_and_rgb_and_joins_idat_chunks():
    from satlas_super_resolution_amd.png_device import parse_png
    seen = set()
    for name, data, pix in PC.corpus():
        info = parse_png(data)
        assert info.reason is None, name
        assert (info.height, info.width) == pix.shape[:2] and info.channels == (1 if pix.ndim == 2 else 3), name
        raw = zlib.decompress(info.stream)                       # many IDAT chunks: one stream
        assert len(raw) == info.height * (info.width * info.channels + 1), name
        seen.add(info.channels)
    assert seen == {1, 3}


def test_parse_png_names_its_reason_and_does_not_raise_for_other_legal_kinds():
    from satlas_super_resolution_amd.png_device import parse_png
    files = PC.refused_files()
    want = {"palette": "palette", "alpha": "alpha", "alpha_la": "alpha", "16-bit": "16-bit", "interlaced": "interlaced"}
    assert set(files) == set(want)
    for key, data in files.items():
        info = parse_png(data)
        assert info.reason == want[key] and info.stream == b"", key


def test_parse_png_raises_on_crc_mismatch_missing_iend_and_bad_signature():
    from satlas_super_resolution_amd.png_device import PngFormatError, parse_png
    name, data, _ = PC.corpus()[0]
    parse_png(data)
    bad = bytearray(data)
    bad[len(data) // 2] ^= 0x10                                  # inside an IDAT payload
    with pytest.raises(PngFormatError, match="CRC"):
        parse_png(bytes(bad))
    with pytest.raises(PngFormatError, match="IEND"):
        parse_png(data[:-12])                                    # the file without its IEND chunk
    with pytest.raises(PngFormatError):
        parse_png(b"GIF89a" + data[6:])
    with pytest.raises(PngFormatError):
        parse_png(data[:40])


def test_host_twin_decodes_the_whole_corpus_in_one_call(lib):
    from satlas_super_resolution_amd.png_device import decode_host, parse_png
    corpus = PC.corpus()
    assert 55 <= len(corpus) <= 70
    infos = [parse_png(data) for _, data, _ in corpus]
    dst, offs, status = decode_host(infos, guard=PC.GUARD)
    assert status.tolist() == [0] * len(corpus), [(corpus[k][0], int(s)) for k, s in enumerate(status) if s]
    for (name, _, pix), o in zip(corpus, offs):
        assert np.array_equal(dst[o:o + pix.size], pix.reshape(-1)), name
    assert _guards_intact(dst, offs, [p.size for _, _, p in corpus], PC.GUARD)


def test_corpus_holds_the_block_kinds_it_claims():
    """the first block of the strategy files: stored / fixed / dynamic, read from the stream's third byte"""
    from satlas_super_resolution_amd.png_device import parse_png
    kinds = {}
    for name, data, _ in PC.corpus():
        s = parse_png(data).stream
        kinds.setdefault((s[2] >> 1) & 3, []).append(name)
    assert any("level0" in n for n in kinds[0]) and any("fixed" in n for n in kinds[1]) and any("default" in n for n in kinds[2])
    far = dict((n, d) for n, d, _ in PC.corpus())["far_repeat"]
    assert len(parse_png(far).stream) < 30000                    # the second copy of the 24 704-byte block went out as matches


def test_malformed_streams_end_with_a_status_inside_their_range(lib):
    from satlas_super_resolution_amd.png_device import PngInfo, decode_host
    w, h, c, good, bad = PC.malformed_streams()
    assert len(bad) == len(good) + 512
    streams = [good] + bad
    dst, offs, status = decode_host([PngInfo(w, h, c, s, None) for s in streams], guard=PC.GUARD)       # the call returns
    n = w * h * c
    assert _guards_intact(dst, offs, [n] * len(streams), PC.GUARD)
    want = PC.malformed_image().reshape(-1)
    assert status[0] == 0 and np.array_equal(dst[offs[0]:offs[0] + n], want)
    ok_both, refused = 0, 0
    for k, s in enumerate(streams):
        try:
            raw = zlib.decompress(s)
        except zlib.error:
            raw = None
            refused += status[k] != 0
        if raw is not None:                                       # what zlib takes, the decoder takes, with zlib's bytes
            assert status[k] == 0, (k, int(status[k]))
            assert len(raw) == h * (w * c + 1)
            ok_both += 1
            assert np.array_equal(dst[offs[k]:offs[k] + n], want), k
    assert status[1:len(good) + 1].all()                          # every truncation is refused
    assert ok_both >= 1 and refused >= len(good)
    print(f"{len(streams)} streams: zlib and the decoder take {ok_both}, statuses seen {sorted(set(status.tolist()))}")


def test_named_malformed_streams_get_their_status(lib):
    from satlas_super_resolution_amd.png_device import PngInfo, decode_host
    w, h, c, named = PC.named_malformed()
    for s in named.values():
        with pytest.raises(zlib.error):
            zlib.decompress(s)
    _, _, status = decode_host([PngInfo(w, h, c, named[k], None) for k in ("truncated", "stored_nlen", "too_far")])
    assert status.tolist() == [1, 4, 7]


def test_bad_descriptors_are_refused_and_touch_nothing(lib):
    import ctypes as C
    from satlas_super_resolution_amd import hip
    good = zlib.compress(PC.filter_rows(PC.image(4, 4, 3), (0,)))
    src = np.frombuffer(good, np.uint8)
    dst = np.full(256, 0xA5, np.uint8)
    scratch = np.zeros(256, np.uint8)
    cases = [hip.PngItem(0, 0, 0, len(good) + 1, 4, 4, 3), hip.PngItem(0, 256 - 47, 0, len(good), 4, 4, 3),
             hip.PngItem(0, 0, 256 - 51, len(good), 4, 4, 3), hip.PngItem(-1, 0, 0, len(good), 4, 4, 3),
             hip.PngItem(0, 0, 0, len(good), 4, 4, 2), hip.PngItem(0, 0, 0, len(good), 0, 4, 3),
             hip.PngItem(0, 0, 0, len(good), 32768, 32768, 3)]
    items = (hip.PngItem * len(cases))(*cases)
    status = np.zeros(len(cases), np.int32)
    assert lib.ssr_png_decode_host(src.ctypes.data, len(good), C.addressof(items), len(cases), dst.ctypes.data, 256, scratch.ctypes.data,
                                   256, status.ctypes.data) == 0
    assert status.tolist() == [12] * len(cases) and (dst == 0xA5).all()
    assert lib.ssr_png_decode_host(None, 0, C.addressof(items), 1, dst.ctypes.data, 256, scratch.ctypes.data, 256, status.ctypes.data) == -1
    assert lib.ssr_png_decode(None, 0, None, 0, None, 0, None, 0, None, 0, None) == -1          # refused before any launch
    assert lib.ssr_stack_zero_scan(None, 0, None, None, 0, 0, None, None) == -1
    assert lib.ssr_stack_gather(None, 0, None, None, None, 0, 0, None, None, None) == -1
    assert lib.ssr_png_scratch_bytes(32, 416, 3) == (416 * 97 + 15) // 16 * 16 and lib.ssr_png_scratch_bytes(0, 1, 3) == -1


def _write_cases(path):
    from satlas_super_resolution_amd.png_device import parse_png
    with open(path, "wb") as f:
        for _, data, pix in PC.corpus():
            i = parse_png(data)
            f.write(struct.pack("<5i", i.width, i.height, i.channels, len(i.stream), pix.size) + i.stream + pix.tobytes())
        w, h, c, good, bad = PC.malformed_streams()
        for s in bad + list(PC.named_malformed()[3].values()):
            f.write(struct.pack("<5i", w, h, c, len(s), 0) + s)


def test_core_runs_clean_under_address_and_undefined_sanitizers(tmp_path):
    """tools/png_inflate_check.cpp, a stand-alone program built from the same header with -fsanitize=address,undefined, over the
    corpus and the malformed set: exact-size heap blocks, so any access outside an item's ranges is a report"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "png_inflate_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "satlas_super_resolution_amd", "csrc"), os.path.join(ROOT, "tools", "png_inflate_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr:
            pytest.skip("the sanitizer runtime cannot be linked here: " + r.stderr.strip().splitlines()[-1])
        raise AssertionError(r.stderr)
    _write_cases(str(tmp_path / "cases.bin"))
    r = subprocess.run([exe, str(tmp_path / "cases.bin")], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 failed" in r.stdout
