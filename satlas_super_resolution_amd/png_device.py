"""PNG decode on the device (`png_decode: device` of infer_grid): the host reads file bytes and parses the PNG container
(`parse_png`: signature, IHDR, chunk CRCs, the IDAT payloads joined into one zlib stream), the device inflates the streams of a
whole batch side by side and reverses the row filters (ssr_png_decode, csrc/png_decode.hip).  The decoded stacks stay on the
device; the zero test and the frame pick of select_frames run there (ssr_stack_zero_scan, ssr_stack_gather).

What the device takes: 8-bit, non-interlaced grayscale or RGB.  Every other legal PNG gets a named reason from `parse_png` and is
decoded by the caller's host reader; its pixels are uploaded into the slot the device decode would have filled."""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

FRAME = 32 * 32 * 3           # bytes of one frame of a Sentinel-2 stack

STATUS_NAMES = {0: "ok", 1: "truncated input", 2: "bad zlib header", 3: "bad block type", 4: "bad stored LEN/NLEN",
                5: "bad code lengths", 6: "invalid symbol", 7: "distance too far back", 8: "output overrun", 9: "output short",
                10: "bad filter byte", 11: "Adler-32 mismatch", 12: "bad descriptor"}


class PngFormatError(ValueError):
    """not a well-formed PNG file: bad signature, chunk CRC mismatch, missing IHDR / IDAT / IEND"""


class PngDecodeError(RuntimeError):
    """a stream the decoder refused: names the file and the status"""

    def __init__(self, name: str, status: int):
        super().__init__(f"{name}: PNG decode failed with status {status} ({STATUS_NAMES.get(status, 'unknown')})")
        self.name, self.status = name, status


class PngInfo(NamedTuple):
    width: int
    height: int
    channels: int             # 1 or 3 when reason is None
    stream: bytes             # the zlib stream (all IDAT payloads in file order); b"" when reason is not None
    reason: Optional[str]     # None: the device decoder takes the file; else why not: "palette", "alpha", "16-bit", "interlaced", ...


_SIG = b"\x89PNG\r\n\x1a\n"


def parse_png(data: bytes) -> PngInfo:
    """The container of one PNG file.  Raises PngFormatError for a broken file; a legal PNG of a kind the device decoder does not
    take comes back with `reason` set and is never an error."""
    if len(data) < 8 or data[:8] != _SIG:
        raise PngFormatError("not a PNG file (signature)")
    pos, ihdr, idat, end = 8, None, [], False
    n = len(data)
    while pos < n:
        if pos + 12 > n:
            raise PngFormatError("chunk header past the end of the file")
        length, = struct.unpack_from(">I", data, pos)
        tag = data[pos + 4:pos + 8]
        if pos + 12 + length > n:
            raise PngFormatError(f"chunk {tag!r} past the end of the file")
        crc, = struct.unpack_from(">I", data, pos + 8 + length)
        if zlib.crc32(data[pos + 4:pos + 8 + length]) & 0xffffffff != crc:
            raise PngFormatError(f"chunk {tag!r}: CRC mismatch")
        body = data[pos + 8:pos + 8 + length]
        pos += 12 + length
        if ihdr is None:
            if tag != b"IHDR" or length != 13:
                raise PngFormatError("the first chunk is not IHDR")
            ihdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"IEND":
            end = True
            break
    if ihdr is None or not end:
        raise PngFormatError("no IEND chunk" if ihdr is not None else "no IHDR chunk")
    w, h, depth, ctype, comp, filt, interlace = ihdr
    if w < 1 or h < 1 or comp != 0 or filt != 0 or ctype not in (0, 2, 3, 4, 6) or interlace not in (0, 1):
        raise PngFormatError(f"IHDR: {ihdr}")
    if not idat:
        raise PngFormatError("no IDAT chunk")
    reason = None
    if ctype == 3:
        reason = "palette"
    elif ctype in (4, 6):
        reason = "alpha"
    elif depth == 16:
        reason = "16-bit"
    elif depth != 8:
        reason = f"{depth}-bit"
    elif interlace:
        reason = "interlaced"
    elif w > 32768 or h > 32768 or h * (w * (3 if ctype == 2 else 1) + 1) > (1 << 24):
        reason = "too large"
    if reason is not None:
        return PngInfo(w, h, {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype], b"", reason)
    return PngInfo(w, h, 3 if ctype == 2 else 1, idat[0] if len(idat) == 1 else b"".join(idat), None)


def _a16(v: int) -> int:
    return (v + 15) // 16 * 16


def scratch_bytes(info: PngInfo) -> int:
    """raw-scanline bytes the decoder needs for one image (ssr_png_scratch_bytes)"""
    from . import hip
    n = int(hip.lib().ssr_png_scratch_bytes(info.width, info.height, info.channels))
    if n < 0:
        raise ValueError(f"{info.width} x {info.height} x {info.channels}: not an image the device decoder takes")
    return n


def make_items(infos: Sequence[PngInfo], dst_offs: Sequence[int]):
    """(the item table, the concatenated streams with every stream at a multiple of 16, scratch bytes, LDS pool that holds the
    largest item's stream and raw scanlines) for device-decodable infos whose pixels go to dst_offs"""
    from . import hip
    items = (hip.PngItem * max(1, len(infos)))()
    parts, src_off, raw_off, pool = [], 0, 0, 0
    for k, (info, d) in enumerate(zip(infos, dst_offs)):
        assert info.reason is None, info.reason
        items[k] = hip.PngItem(src_off, int(d), raw_off, len(info.stream), info.width, info.height, info.channels)
        pad = _a16(len(info.stream)) - len(info.stream)
        parts.append(info.stream)
        if pad:
            parts.append(bytes(pad))
        src_off += len(info.stream) + pad
        raw_off += scratch_bytes(info)
        pool = max(pool, _a16(len(info.stream)) + scratch_bytes(info))
    return items, b"".join(parts), raw_off, pool


class Batch:
    """one decode in flight: the device buffer of decoded images, where each lies, and the statuses on their way down"""

    def __init__(self, names, buf, offs, sizes, idx, status_host, event, keep):
        self.names, self.buf, self.offs, self.sizes = list(names), buf, list(offs), list(sizes)
        self._idx, self._status_host, self._event, self._keep = idx, status_host, event, keep
        self.offs_dev = self.T_dev = self.has_zero_host = None
        self.T: List[int] = []

    def statuses(self) -> np.ndarray:
        """waits for the batch; int32 per file, 0 for a file the host reader decoded"""
        self._event.synchronize()
        st = np.zeros(len(self.names), np.int32)
        if self._idx:
            st[self._idx] = self._status_host.numpy()[:len(self._idx)]
        return st

    def wait(self) -> np.ndarray:
        """the statuses, all zero: raises PngDecodeError for the first file whose status is not"""
        st = self.statuses()
        bad = np.flatnonzero(st)
        if bad.size:
            raise PngDecodeError(self.names[int(bad[0])], int(st[bad[0]]))
        self._keep = None
        return st


def launch_decode(names: Sequence[str], infos: Sequence[PngInfo], fallbacks: Optional[Sequence[Optional[np.ndarray]]] = None,
                  device=None, scan_frames: bool = False, guard: int = 0, lds_pool: Optional[int] = None) -> Batch:
    """Enqueue (on the current stream; nothing waits) the upload of a batch from pinned memory, its decode, and the download of the
    statuses.  File k's pixels land at `offs[k]` of one uint8 device buffer, tight [H, W, C]; `fallbacks[k]` is the host-decoded
    array of a file `parse_png` gave a reason for, uploaded into its place.  scan_frames: every image is taken as a stack of
    32 x 32 x 3 frames (its bytes / 3072) and the zero test of select_frames runs behind the decode; `has_zero_host` ([B, Tmax],
    pinned) comes down with the statuses.  guard: bytes left between the images (tests fill and check them).  lds_pool: the LDS a
    block gets for an item's stream and raw scanlines (default: what the batch's largest item needs, up to the device's limit; 0:
    everything through global memory)."""
    import torch
    from . import hip
    device = torch.device("cuda") if device is None else torch.device(device)
    B = len(infos)
    assert B > 0 and len(names) == B
    sizes, offs, dst_len = [], [], guard
    for k, info in enumerate(infos):
        if info.reason is None:
            nb = info.width * info.height * info.channels
        else:
            if fallbacks is None or fallbacks[k] is None:
                raise ValueError(f"{names[k]}: {info.reason} PNG and no host-decoded array given")
            nb = int(fallbacks[k].nbytes)
        sizes.append(nb)
        offs.append(dst_len)
        dst_len += _a16(nb) + guard
    idx = [k for k in range(B) if infos[k].reason is None]
    items, streams, scratch_len, pool = make_items([infos[k] for k in idx], [offs[k] for k in idx])
    pool = min(pool if lds_pool is None else int(lds_pool), int(hip.lib().ssr_png_lds_pool_max()))
    T = [nb // FRAME for nb in sizes]
    if scan_frames:
        for k, nb in enumerate(sizes):
            if nb % FRAME or nb == 0:
                raise ValueError(f"{names[k]}: {nb} bytes of pixels are not a stack of 32 x 32 x 3 frames")
    # one pinned block, one copy: [offs int64 B][T int32 B][item table][streams][host-decoded pixels]
    head = np.concatenate([np.asarray(offs, np.int64).view(np.uint8), np.asarray(T, np.int32).view(np.uint8)])
    table = bytes(memoryview(items).cast("B"))[:40 * len(idx)]
    o_T, o_items = 8 * B, _a16(12 * B)
    o_streams = o_items + _a16(len(table))
    o_fb = o_streams + len(streams)
    fb_offs, total = {}, o_fb
    for k in range(B):
        if infos[k].reason is not None:
            fb_offs[k] = total
            total += _a16(sizes[k])
    pin = torch.empty(max(16, total), dtype=torch.uint8, pin_memory=True)
    pn = pin.numpy()
    pn[:12 * B] = head
    pn[o_items:o_items + len(table)] = np.frombuffer(table, np.uint8)
    pn[o_streams:o_fb] = np.frombuffer(streams, np.uint8)
    for k, o in fb_offs.items():
        pn[o:o + sizes[k]] = np.ascontiguousarray(fallbacks[k], dtype=np.uint8).reshape(-1)
    up = pin.to(device, non_blocking=True)
    buf = torch.empty(dst_len, dtype=torch.uint8, device=device)
    scratch = torch.empty(max(16, scratch_len), dtype=torch.uint8, device=device)
    status = torch.zeros(max(1, len(idx)), dtype=torch.int32, device=device)
    if guard:
        buf.fill_(0xA5)
    if idx:
        hip.check(hip.lib().ssr_png_decode(up.data_ptr() + o_streams, len(streams), up.data_ptr() + o_items, len(idx), buf.data_ptr(),
                                           dst_len, scratch.data_ptr(), scratch.numel(), status.data_ptr(), pool, hip.stream_ptr()),
                  "ssr_png_decode")
    for k, o in fb_offs.items():
        buf[offs[k]:offs[k] + sizes[k]].copy_(up[o:o + sizes[k]])
    status_host = torch.empty(status.shape, dtype=torch.int32, pin_memory=True)
    status_host.copy_(status, non_blocking=True)
    batch = Batch(names, buf, offs, sizes, idx, status_host, None, (pin, up, scratch, status))
    batch.T = T
    batch.offs_dev = up[:8 * B].view(torch.int64)
    batch.T_dev = up[o_T:o_T + 4 * B].view(torch.int32)
    if scan_frames:
        hz = stack_zero_scan(buf, batch.offs_dev, batch.T_dev, max(T))
        batch.has_zero_host = torch.empty(hz.shape, dtype=torch.uint8, pin_memory=True)
        batch.has_zero_host.copy_(hz, non_blocking=True)
    batch._event = torch.cuda.Event()
    batch._event.record()
    return batch


def decode_batch(names: Sequence[str], infos: Sequence[PngInfo], fallbacks=None, device=None, guard: int = 0):
    """Upload the streams from pinned memory, decode them on the device, wait.  Returns (the device buffer, the byte offset of every
    image in it, the statuses); a non-zero status raises PngDecodeError naming the file and the status before anything is returned."""
    b = launch_decode(names, infos, fallbacks, device, guard=guard)
    st = b.wait()
    return b.buf, b.offs, st


def stack_zero_scan(buf, offs_dev, T_dev, Tmax: int):
    """has_zero uint8 [B, Tmax] on the device for the stacks [T_b, 32, 32, 3] at offs_dev (int64) of buf; 0 beyond T_b"""
    import torch
    from . import hip
    B = int(offs_dev.numel())
    hz = torch.empty(B, Tmax, dtype=torch.uint8, device=buf.device)
    hip.check(hip.lib().ssr_stack_zero_scan(buf.data_ptr(), buf.numel(), offs_dev.data_ptr(), T_dev.data_ptr(), B, Tmax, hz.data_ptr(),
                                            hip.stream_ptr()), "ssr_stack_zero_scan")
    return hz


def stack_gather(buf, offs_dev, T_dev, frame_ids):
    """(uint8 [B, n, 32, 32, 3] of frames frame_ids[b, k] (int32, device), uint8 [B, 32, 32, 3] of every stack's frame 0)"""
    import torch
    from . import hip
    B, n = frame_ids.shape
    out = torch.empty(B, n, 32, 32, 3, dtype=torch.uint8, device=buf.device)
    first = torch.empty(B, 32, 32, 3, dtype=torch.uint8, device=buf.device)
    hip.check(hip.lib().ssr_stack_gather(buf.data_ptr(), buf.numel(), offs_dev.data_ptr(), T_dev.data_ptr(), frame_ids.data_ptr(), B, n,
                                         out.data_ptr(), first.data_ptr(), hip.stream_ptr()), "ssr_stack_gather")
    return out, first


def decode_host(infos: Sequence[PngInfo], guard: int = 0):
    """The CPU twin (ssr_png_decode_host: the same decoder text compiled for the host) on numpy buffers.  Returns (dst uint8 with
    `guard` bytes of 0xA5 around every image, the offsets, the statuses); no exception for a bad stream."""
    from . import hip
    sizes = [i.width * i.height * i.channels for i in infos]
    offs, dst_len = [], guard
    for nb in sizes:
        offs.append(dst_len)
        dst_len += _a16(nb) + guard
    items, streams, scratch_len, _ = make_items(infos, offs)
    dst = np.full(max(1, dst_len), 0xA5, np.uint8)
    src = np.frombuffer(streams, np.uint8) if streams else np.zeros(1, np.uint8)
    scratch = np.zeros(max(16, scratch_len), np.uint8)
    status = np.full(len(infos), -1, np.int32)
    rc = hip.lib().ssr_png_decode_host(src.ctypes.data, len(streams), C.addressof(items), len(infos), dst.ctypes.data, dst_len,
                                       scratch.ctypes.data, scratch_len, status.ctypes.data)
    hip.check(rc, "ssr_png_decode_host")
    return dst, offs, status
