"""GPU: the batched PNG decoder (ssr_png_decode, csrc/png_decode.hip) and the stack kernels behind `png_decode: device`.  Exact byte
equality everywhere: against Pillow for files, against the host twin (the same decoder text on the CPU) for statuses, against numpy
for the zero scan and the frame gather."""
import numpy as np
import pytest
import torch

import png_corpus as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parsed():
    from satlas_super_resolution_amd.png_device import parse_png
    corpus = PC.corpus()
    return corpus, [parse_png(data) for _, data, _ in corpus]


def _check(batch, pixels):
    """statuses 0, every image equal to its expected pixels, every byte between the images still 0xA5"""
    assert batch.statuses().tolist() == [0] * len(pixels)
    got = batch.buf.cpu().numpy()
    mask = np.ones(got.shape, bool)
    for k, (o, pix) in enumerate(zip(batch.offs, pixels)):
        assert np.array_equal(got[o:o + pix.size], pix.reshape(-1)), batch.names[k]
        mask[o:o + pix.size] = False
    assert (got[mask] == 0xA5).all()
    return got


@pytest.mark.parametrize("lds_pool", [None, 0, 24 * 1024])      # everything in LDS / everything through global memory / mixed per item
def test_one_launch_over_the_whole_corpus_equals_pillow(parsed, lds_pool):
    from satlas_super_resolution_amd.png_device import launch_decode
    corpus, infos = parsed
    assert 55 <= len(corpus) <= 70
    b = launch_decode([n for n, _, _ in corpus], infos, guard=PC.GUARD, lds_pool=lds_pool)
    _check(b, [p for _, _, p in corpus])


@pytest.mark.parametrize("n", [1, 257])
def test_launches_of_one_and_of_257_items(parsed, n):
    from satlas_super_resolution_amd.png_device import launch_decode
    corpus, infos = parsed
    k = next(k for k, (_, _, p) in enumerate(corpus) if p.shape == (32, 32, 3))
    b = launch_decode([f"{corpus[k][0]}#{i}" for i in range(n)], [infos[k]] * n, guard=PC.GUARD)
    _check(b, [corpus[k][2]] * n)


def test_a_second_launch_gives_the_same_bytes(parsed):
    from satlas_super_resolution_amd.png_device import launch_decode
    corpus, infos = parsed
    names = [n for n, _, _ in corpus]
    a = launch_decode(names, infos, guard=PC.GUARD)
    b = launch_decode(names, infos, guard=PC.GUARD)
    assert a.statuses().tolist() == b.statuses().tolist() == [0] * len(corpus)
    assert torch.equal(a.buf, b.buf)


def test_malformed_items_among_good_ones_get_the_host_twins_statuses(parsed):
    """a truncated stream, a bad stored LEN/NLEN and a distance too far back in one launch with good items"""
    from satlas_super_resolution_amd.png_device import PngDecodeError, PngInfo, decode_host, launch_decode
    corpus, infos = parsed
    w, h, c, named = PC.named_malformed()
    good = [0, 9, 20, 40]
    mixed = [infos[good[0]], PngInfo(w, h, c, named["truncated"], None), infos[good[1]], PngInfo(w, h, c, named["stored_nlen"], None),
             infos[good[2]], PngInfo(w, h, c, named["too_far"], None), infos[good[3]]]
    names = [f"item{k}" for k in range(len(mixed))]
    _, _, host = decode_host(mixed)
    assert host.tolist() == [0, 1, 0, 4, 0, 7, 0]
    b = launch_decode(names, mixed, guard=PC.GUARD)
    assert b.statuses().tolist() == host.tolist()
    got = b.buf.cpu().numpy()
    mask = np.ones(got.shape, bool)
    for k, (o, n) in enumerate(zip(b.offs, b.sizes)):
        mask[o:o + n] = False
        if k % 2 == 0:                                   # the good items are unaffected
            pix = corpus[good[k // 2]][2]
            assert np.array_equal(got[o:o + n], pix.reshape(-1)), k
    assert (got[mask] == 0xA5).all()                     # and nobody wrote outside its range
    with pytest.raises(PngDecodeError, match="item1.*status 1"):
        b.wait()


def test_stack_zero_scan_and_gather_equal_numpy():
    """T in {1, 8, 13} mixed in one batch; stacks with zero samples in no frame, in some frames, in all frames"""
    from satlas_super_resolution_amd.png_device import FRAME, stack_gather, stack_zero_scan
    rng = np.random.default_rng(3)
    Ts = [13, 1, 8, 13, 8, 1, 13, 8]
    kinds = ["none", "none", "some", "some", "all", "all", "all", "none"]
    stacks, offs, pos = [], [], 16
    for T, kind in zip(Ts, kinds):
        s = rng.integers(1, 256, (T, 32, 32, 3), dtype=np.uint8)
        frames = {"none": [], "some": list(range(0, T, 3)), "all": list(range(T))}[kind]
        for t in frames:                                 # one zero sample at a different place of every frame, incl. first and last byte
            s[t].reshape(-1)[(t * 1021) % FRAME if t % 4 else (0 if t % 8 else FRAME - 1)] = 0
        stacks.append(s)
        offs.append(pos)
        pos += T * FRAME + (16 if len(offs) % 2 else 4)  # some stacks 16-byte aligned, some only 4-byte
    host = np.full(pos, 7, np.uint8)
    for s, o in zip(stacks, offs):
        host[o:o + s.size] = s.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    offs_dev, T_dev = torch.tensor(offs, dtype=torch.int64).cuda(), torch.tensor(Ts, dtype=torch.int32).cuda()
    hz = stack_zero_scan(buf, offs_dev, T_dev, 13).cpu().numpy()
    want = np.zeros((len(Ts), 13), np.uint8)
    for b, s in enumerate(stacks):
        want[b, :len(s)] = (s == 0).any(axis=(1, 2, 3))
    assert np.array_equal(hz, want)
    assert want[2].sum() == 3 and want[4, :8].all() and not want[4, 8:].any() and not want[0].any()
    n = 3
    ids = np.stack([rng.integers(0, T, n) for T in Ts]).astype(np.int32)
    ids[0] = [12, 0, 12]                                 # repeats and the last frame
    out, first = stack_gather(buf, offs_dev, T_dev, torch.from_numpy(ids).cuda())
    out, first = out.cpu().numpy(), first.cpu().numpy()
    assert out.shape == (len(Ts), n, 32, 32, 3) and first.shape == (len(Ts), 32, 32, 3)
    for b, s in enumerate(stacks):
        assert np.array_equal(out[b], s[ids[b]]), b
        assert np.array_equal(first[b], s[0]), b
