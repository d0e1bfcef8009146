"""JPEG frames decoded on the device (include/syncfusion_amd.h, "JPEG frames on the device").

``decode_jpeg_batch`` takes the bytes of N equally sized JPEG files and returns the ``(N, H, W, 3)`` uint8 tensor
``PIL.Image.open(f).convert("RGB")`` gives for each of them, byte for byte: the host parses the markers (``sf_jpeg_parse``), the file
bytes go to the device in one copy together with the descriptors and the segment table, and three HIP kernels do the rest (Huffman
decode, integer IDCT, fancy chroma upsampling, integer YCbCr -> RGB: libjpeg's default decode path).  The equality holds for baseline
files as an encoder writes them (SOF0 / 8-bit SOF1, one interleaved scan, one or three components, 4:4:4 / 4:2:2 / 4:2:0).  What the
kernels do not cover -- progressive, arithmetic-coded, lossless or 12-bit frames, 2 or 4 components, several scans, Huffman table ids
above 1, other sampling factors (h1v2 included), an Adobe marker with transform != 1, component ids ``R G B`` -- is reported by the parser
with its reason, and that file is decoded by Pillow into its slot (``fallback="pil"``) or refused (``fallback="raise"``).
"""
from __future__ import annotations

import ctypes as C
import io
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import JpegDesc, JpegSegment, SyncFusionAmdError

Tensor = torch.Tensor

JPEG_OK, JPEG_UNSUPPORTED, JPEG_MALFORMED = 0, 1, 2
SF_ERR_INVALID, SF_ERR_WORKSPACE = 1, 5               # include/syncfusion_amd.h
MAX_BATCH = 65535                                     # files per call (sf_jpeg_parse refuses more)
STATUS_NAMES = {0: "ok", 1: "out of bits", 2: "invalid Huffman code", 3: "coefficient index overflow", 4: "trailing bytes in a segment",
                5: "bad segment table entry"}
_ALIGN = 256
_DESC_BYTES, _SEG_BYTES = C.sizeof(JpegDesc), C.sizeof(JpegSegment)


@dataclass
class JpegInfo:
    """What ``sf_jpeg_parse`` says about one file.  ``supported``: the device kernels decode it; otherwise ``reason`` says why not."""
    width: int
    height: int
    components: int
    sampling: List[Tuple[int, int]]                 # (h, v) per component
    quant_selectors: List[int]
    dc_selectors: List[int]
    ac_selectors: List[int]
    quant_tables: dict                              # id -> (64,) uint16 in natural order
    quant_precision: dict                           # id -> 8 or 16
    huffman_tables: dict                            # ("dc" | "ac", id) -> (counts (16,) uint8, values (n,) uint8)
    restart_interval: int
    mcus: Tuple[int, int]                           # (across, down)
    data_range: Tuple[int, int]                     # entropy-coded bytes [begin, end) in the file
    segments: List[Tuple[int, int, int, int]] = field(default_factory=list)   # (first_mcu, mcu_count, byte_begin, byte_end)
    supported: bool = True
    reason: str = ""


def _as_bytes(b) -> bytes:
    if isinstance(b, (bytes, bytearray, memoryview)):
        return bytes(b)
    if isinstance(b, np.ndarray):
        return b.tobytes()
    if isinstance(b, torch.Tensor):
        return b.cpu().numpy().tobytes()
    raise TypeError(f"JPEG bytes expected, got {type(b).__name__}")


def _info(d: JpegDesc, segs, base: int) -> JpegInfo:
    nc = d.ncomp if d.ncomp in (1, 3) else 0
    q = {i: np.array(d.quant[i], dtype=np.uint16) for i in range(4) if d.quant_precision[i] >= 0}
    huff = {}
    for slot in range(4):
        if d.huff_present & (1 << slot):
            counts = np.array(d.huff_counts[slot], dtype=np.uint8)
            huff[("dc" if slot < 2 else "ac", slot & 1)] = (counts, np.array(d.huff_values[slot], dtype=np.uint8)[: int(counts.sum())])
    return JpegInfo(width=d.width, height=d.height, components=d.ncomp, sampling=[(d.h[c], d.v[c]) for c in range(nc)],
                    quant_selectors=[d.tq[c] for c in range(nc)], dc_selectors=[d.td[c] for c in range(nc)],
                    ac_selectors=[d.ta[c] for c in range(nc)], quant_tables=q,
                    quant_precision={i: 16 if d.quant_precision[i] else 8 for i in q}, huffman_tables=huff,
                    restart_interval=d.restart_interval, mcus=(d.mcus_x, d.mcus_y), data_range=(d.data_begin - base, d.data_end - base),
                    segments=[(s.first_mcu, s.mcu_count, s.byte_begin - base, s.byte_end - base) for s in segs],
                    supported=d.status == JPEG_OK, reason=d.reason.decode("ascii", "replace"))


def parse_jpeg(blob) -> JpegInfo:
    """The descriptor and the segment table of one JPEG file (host only; works without a GPU).  A stream outside the device kernels'
    coverage comes back with ``supported=False`` and its ``reason``; a malformed header raises ``SyncFusionAmdError``."""
    lib = _lib.load()
    data = _as_bytes(blob)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    offsets = (C.c_int64 * 2)(0, len(data))
    desc = JpegDesc()
    n = C.c_int64(0)
    _lib.check(lib.sf_jpeg_parse(buf, offsets, 1, C.byref(desc), None, 0, C.byref(n)), "sf_jpeg_parse")
    segs = (JpegSegment * max(1, n.value))()
    _lib.check(lib.sf_jpeg_parse(buf, offsets, 1, C.byref(desc), segs, n.value, C.byref(n)), "sf_jpeg_parse")
    return _info(desc, segs[: n.value], 0)


class _Staged:
    """The pinned staging buffer of one batch: [ file bytes | descriptors | segment table ], each part at a 256-byte boundary."""

    def __init__(self, blobs: Sequence[bytes], pin: bool):
        lib = _lib.load()
        self.n = len(blobs)
        if not 1 <= self.n <= MAX_BATCH:
            raise ValueError(f"a batch holds 1 .. {MAX_BATCH} files, got {self.n}")
        sizes = [len(b) for b in blobs]
        self.offsets = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(sizes, out=self.offsets[1:])
        self.n_bytes = int(self.offsets[-1])
        self.desc_at = -(-max(1, self.n_bytes) // _ALIGN) * _ALIGN
        self.seg_at = self.desc_at + -(-self.n * _DESC_BYTES // _ALIGN) * _ALIGN
        capacity = max(64, 2 * self.n)
        while True:
            self.host = torch.empty(self.seg_at + capacity * _SEG_BYTES, dtype=torch.uint8, pin_memory=pin)
            view = self.host.numpy()
            for b, o in zip(blobs, self.offsets[:-1]):
                view[o: o + len(b)] = np.frombuffer(b, dtype=np.uint8)
            view[self.n_bytes: self.desc_at] = 0
            base = self.host.data_ptr()
            n = C.c_int64(0)
            self.rc = lib.sf_jpeg_parse(base, self.offsets.ctypes.data, self.n, base + self.desc_at, base + self.seg_at, capacity, C.byref(n))
            self.n_segs = int(n.value)
            if self.rc == SF_ERR_WORKSPACE and self.n_segs > capacity:        # SF_ERR_WORKSPACE: more restart intervals than the first guess
                capacity = self.n_segs
                continue
            break
        self.used = self.seg_at + self.n_segs * _SEG_BYTES
        self.desc = (JpegDesc * self.n).from_address(base + self.desc_at)
        # SF_ERR_INVALID with a malformed file among them: its descriptor says so, and the caller decides what becomes of it
        if self.rc != 0 and not (self.rc == SF_ERR_INVALID and any(d.status == JPEG_MALFORMED for d in self.desc)):
            _lib.check(self.rc, "sf_jpeg_parse")


def _pil_rgb(blob: bytes) -> np.ndarray:
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


def decode_jpeg_batch(blobs: Sequence, device="cuda", fallback: str = "pil", check: bool = True) -> Union[Tensor, Tuple[Tensor, Tensor]]:
    """N JPEG files (bytes) of one size -> ``(N, H, W, 3)`` uint8 on ``device``, equal to Pillow's ``convert("RGB")``.

    ``fallback``: what happens to a file the kernels do not cover (module docstring) -- ``"pil"``: Pillow decodes it into its slot;
    ``"raise"``: ``SyncFusionAmdError`` naming the file and the reason.  ``check=True`` reads the per-file status words of the entropy
    decoder back (one small copy): a flagged file goes to Pillow (``"pil"``; a truly broken file then raises Pillow's own error) or raises
    (``"raise"``).  ``check=False`` returns ``(frames, status)`` without synchronising; ``status`` is the (N,) int32 device tensor."""
    if fallback not in ("pil", "raise"):
        raise ValueError("fallback: 'pil' or 'raise'")
    lib = _lib.load()
    device = torch.device(device)
    _lib.require_gpu_tensor(torch.empty(0, device=device), "decode_jpeg_batch")
    blobs = [_as_bytes(b) for b in blobs]
    if not blobs:
        raise ValueError("no frames")
    st = _Staged(blobs, pin=True)
    desc = st.desc
    todo = [i for i in range(st.n) if desc[i].status != JPEG_OK]
    if todo and fallback == "raise":
        i = todo[0]
        kind = "malformed" if desc[i].status == JPEG_MALFORMED else "not supported on the device"
        raise SyncFusionAmdError(f"decode_jpeg_batch: file {i} is {kind}: {desc[i].reason.decode('ascii', 'replace')}")
    host_frames = {i: _pil_rgb(blobs[i]) for i in todo}        # (Pillow raises its own error for a broken file)
    sizes = {(desc[i].height, desc[i].width) for i in range(st.n) if desc[i].status == JPEG_OK} | {a.shape[:2] for a in host_frames.values()}
    if len(sizes) != 1:
        raise ValueError(f"frames of one batch differ in size: {sorted(sizes)}")
    (H, W), = sizes
    with torch.cuda.device(device):
        dev = st.host[: st.used].to(device, non_blocking=True)                      # THE upload
        ws_bytes = int(lib.sf_jpeg_decode_workspace_bytes(C.addressof(desc), st.n))
        if ws_bytes < 0:
            raise SyncFusionAmdError("sf_jpeg_decode_workspace_bytes: bad descriptors")
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=device)
        out = torch.empty((st.n, H, W, 3), dtype=torch.uint8, device=device)
        status = torch.empty(st.n, dtype=torch.int32, device=device)
        base = dev.data_ptr()
        _lib.check(lib.sf_jpeg_decode(base, st.n_bytes, C.addressof(desc), base + st.desc_at, base + st.seg_at, st.n_segs, st.n, H, W,
                                      out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(device)), "sf_jpeg_decode")
        if host_frames:
            idx = sorted(host_frames)
            out[torch.tensor(idx, device=device)] = torch.from_numpy(np.stack([host_frames[i] for i in idx])).to(device)
        if not check:
            return out, status
        flagged = torch.nonzero(status).flatten().tolist()     # the one small copy
        if flagged and fallback == "raise":
            i = flagged[0]
            code = int(status[i])
            raise SyncFusionAmdError(f"decode_jpeg_batch: file {i}: entropy decoder status {code} ({STATUS_NAMES.get(code, '?')})")
        if flagged:
            out[torch.tensor(flagged, device=device)] = torch.from_numpy(np.stack([_pil_rgb(blobs[i]) for i in flagged])).to(device)
    return out


def read_files(paths: Sequence[str]) -> List[bytes]:
    out = []
    for p in paths:
        with open(p, "rb") as f:
            out.append(f.read())
    return out
