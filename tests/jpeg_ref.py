"""libjpeg's default decode path restated in numpy: marker parser, Huffman decode, the integer "islow" IDCT, fancy h2v1 / h2v2 chroma
upsampling and integer YCbCr -> RGB.  The reference of the JPEG tests: ``decode(data)`` returns the coefficient planes (int16, natural
order, padded to whole MCUs) and the RGB image, which equals ``PIL.Image.open(...).convert("RGB")`` byte for byte
(test_jpeg_cpu.py asserts that before anything is compared with it).

Plain module (not a conftest); covers what the device decoder covers: baseline / 8-bit extended sequential frames, one interleaved
scan, one or three components, luma 1x1 / 2x1 / 2x2 over 1x1 chroma.
"""
from __future__ import annotations

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Unsupported(Exception):
    pass


def parse(data: bytes) -> dict:
    """Markers up to the first scan, then the extent of the entropy-coded data and its restart segments."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    info = dict(quant={}, quant_precision={}, huff={}, restart_interval=0, unsupported=None)
    pos = 2
    while True:
        if data[pos] != 0xFF:
            raise ValueError("marker expected")
        while data[pos] == 0xFF:
            pos += 1
        m = data[pos]
        pos += 1
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        n = (data[pos] << 8) | data[pos + 1]
        seg = data[pos + 2: pos + n]
        pos += n
        if m == 0xDB:
            k = 0
            while k < len(seg):
                prec, tid = seg[k] >> 4, seg[k] & 15
                k += 1
                raw = np.frombuffer(seg[k: k + (128 if prec else 64)], dtype=">u2" if prec else np.uint8).astype(np.uint16)
                k += 128 if prec else 64
                q = np.zeros(64, dtype=np.uint16)
                q[ZIGZAG] = raw
                info["quant"][tid] = q
                info["quant_precision"][tid] = 16 if prec else 8
        elif m == 0xC4:
            k = 0
            while k < len(seg):
                cls, tid = seg[k] >> 4, seg[k] & 15
                counts = np.frombuffer(seg[k + 1: k + 17], dtype=np.uint8).copy()
                total = int(counts.sum())
                info["huff"][("dc" if cls == 0 else "ac", tid)] = (counts, np.frombuffer(seg[k + 17: k + 17 + total], dtype=np.uint8).copy())
                k += 17 + total
        elif m == 0xDD:
            info["restart_interval"] = (seg[0] << 8) | seg[1]
        elif 0xC0 <= m <= 0xCF and m not in (0xC8, 0xCC):
            if m not in (0xC0, 0xC1) or seg[0] != 8:
                info["unsupported"] = f"SOF{m - 0xC0} / {seg[0]} bits"
            info["height"], info["width"], nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            info["components"] = nc
            info["ids"] = [seg[6 + 3 * i] for i in range(nc)]
            info["sampling"] = [(seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15) for i in range(nc)]
            info["tq"] = [seg[8 + 3 * i] for i in range(nc)]
            if nc == 1:
                info["sampling"] = [(1, 1)]
            elif nc != 3:
                info["unsupported"] = f"{nc} components"
        elif m == 0xDA:
            ns = seg[0]
            if ns != info["components"]:
                info["unsupported"] = "several scans"
            info["td"] = [seg[2 + 2 * i] >> 4 for i in range(ns)]
            info["ta"] = [seg[2 + 2 * i] & 15 for i in range(ns)]
            break
    begin = pos
    end = len(data)
    k = begin
    while True:
        k = data.find(b"\xff", k)
        if k < 0 or k + 1 >= len(data):
            break
        if data[k + 1] == 0 or 0xD0 <= data[k + 1] <= 0xD7:
            k += 2
            continue
        if data[k + 1] == 0xFF:
            k += 1
            continue
        end = k
        break
    info["data_range"] = (begin, end)
    if info["unsupported"] is None:
        (h0, v0) = info["sampling"][0]
        if info["components"] == 3 and (info["sampling"][1:] != [(1, 1), (1, 1)] or (h0, v0) not in ((1, 1), (2, 1), (2, 2))):
            info["unsupported"] = f"sampling {info['sampling']}"
    if info["unsupported"] is None:
        mx, my = -(-info["width"] // (8 * h0)), -(-info["height"] // (8 * v0))
        info["mcus"] = (mx, my)
        ri = info["restart_interval"] or mx * my
        nseg = -(-mx * my // ri)
        segs, q = [], begin
        for s in range(nseg):
            first = s * ri
            count = min(ri, mx * my - first)
            if s + 1 == nseg:
                segs.append((first, count, q, end))
                break
            k = q
            while True:
                k = data.find(b"\xff", k, end)
                assert k >= 0, "restart marker missing"
                if 0xD0 <= data[k + 1] <= 0xD7:
                    break
                k += 2 if data[k + 1] == 0 else 1
            segs.append((first, count, q, k))
            q = k + 2
        info["segments"] = segs
    return info


def _huff_lut(counts, values):
    """16-bit window -> (length, symbol); length 0: no code."""
    lens = np.zeros(65536, dtype=np.int32)
    syms = np.zeros(65536, dtype=np.int32)
    code, k = 0, 0
    for l in range(1, 17):
        for _ in range(int(counts[l - 1])):
            lo = code << (16 - l)
            lens[lo: lo + (1 << (16 - l))] = l
            syms[lo: lo + (1 << (16 - l))] = int(values[k])
            code += 1
            k += 1
        code <<= 1
    return lens.tolist(), syms.tolist()


PAD_BYTES = 512        # zeros behind a segment: more than one block can consume (64 symbols of at most 16 + 15 bits)
ST_OUT_OF_BITS, ST_BAD_CODE, ST_INDEX_OVERFLOW, ST_TRAILING_BYTES = 1, 2, 3, 4


def _windows(segment: bytes, pad: int):
    """The 16-bit window at every bit position of the unstuffed segment (zeros behind its end)."""
    raw = segment.replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(raw + b"\0" * pad, dtype=np.uint8)).astype(np.int32)
    n = len(bits) - 16
    win = np.zeros(n, dtype=np.int32)
    for i in range(16):
        win |= bits[i: i + n] << (15 - i)
    return win.tolist(), len(raw) * 8


def _entropy(data: bytes, info: dict, planes, pad: int = PAD_BYTES):
    """Walks every segment into `planes`; returns 0 or the status code of the first problem in segment order, as the decoder under test
    defines them: checked per block (a bad code or an index overflow inside the block first, then bits consumed behind the segment's
    end), and whole bytes left behind the last block of a segment.  Streams whose segments hold a marker are outside this restatement."""
    mx, my = info["mcus"]
    nc = info["components"]
    luts = {key: _huff_lut(*tab) for key, tab in info["huff"].items()}
    zz = ZIGZAG.tolist()
    for first, count, b0, b1 in info["segments"]:
        win, nbits = _windows(data[b0:b1], pad)
        pos = 0
        pred = [0] * nc
        for m in range(first, first + count):
            ym, xm = divmod(m, mx)
            for c in range(nc):
                h, v = info["sampling"][c]
                dlen, dsym = luts[("dc", info["td"][c])]
                alen, asym = luts[("ac", info["ta"][c])]
                for by in range(v):
                    for bx in range(h):
                        blk = planes[c][ym * v + by, xm * h + bx]
                        w = win[pos]
                        if not dlen[w] or dsym[w] > 15:
                            return ST_BAD_CODE
                        s = dsym[w]
                        pos += dlen[w]
                        if s:
                            val = win[pos] >> (16 - s)
                            pos += s
                            pred[c] += val if val >= (1 << (s - 1)) else val - (1 << s) + 1
                        blk[0] = ((pred[c] + 32768) & 0xFFFF) - 32768
                        k = 1
                        while k < 64:
                            w = win[pos]
                            if not alen[w]:
                                return ST_BAD_CODE
                            rs = asym[w]
                            pos += alen[w]
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                return ST_INDEX_OVERFLOW
                            val = win[pos] >> (16 - s)
                            pos += s
                            blk[zz[k]] = val if val >= (1 << (s - 1)) else val - (1 << s) + 1
                            k += 1
                        if pos > nbits:
                            return ST_OUT_OF_BITS
        if (nbits - pos) // 8 > 0:
            return ST_TRAILING_BYTES
    return 0


def _empty_planes(info):
    mx, my = info["mcus"]
    return [np.zeros((my * v, mx * h, 64), dtype=np.int16) for (h, v) in info["sampling"]]


def decode_coefficients(data: bytes, info: dict = None):
    """One (blocks_down, blocks_across, 64) int16 array per component: natural order, padded to whole MCUs."""
    info = info or parse(data)
    if info["unsupported"]:
        raise Unsupported(info["unsupported"])
    planes = _empty_planes(info)
    try:
        status = _entropy(data, info, planes, 8)          # (a clean stream never looks far behind its end)
    except IndexError:
        status = ST_OUT_OF_BITS
    assert status == 0, f"entropy decode status {status}"
    return planes


def entropy_status(data: bytes) -> int:
    """The status word the entropy decoder must report for a (possibly corrupted) supported stream; 0: clean."""
    info = parse(data)
    if info["unsupported"]:
        raise Unsupported(info["unsupported"])
    return _entropy(data, info, _empty_planes(info))


def _idct_pass(x, shift):
    """jidctint's 1-D pass along the last axis of an int64 array."""
    in0, in1, in2, in3, in4, in5, in6, in7 = (x[..., i] for i in range(8))
    z1 = (in2 + in6) * 4433
    t2 = z1 - in6 * 15137
    t3 = z1 + in2 * 6270
    t0 = (in0 + in4) << 13
    t1 = (in0 - in4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = in7, in5, in3, in1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3 = z3 * -16069 + z5
    z4 = z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)
    return (out + (1 << (shift - 1))) >> shift


def idct_planes(coefs, info):
    """uint8 sample planes of the padded extent."""
    out = []
    for c, p in enumerate(coefs):
        bh, bw, _ = p.shape
        x = p.astype(np.int64).reshape(bh, bw, 8, 8) * info["quant"][info["tq"][c]].astype(np.int64).reshape(8, 8)
        x = _idct_pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)      # pass 1: columns
        x = _idct_pass(x, 18)                                        # pass 2: rows
        x = np.clip(x + 128, 0, 255).astype(np.uint8)
        out.append(x.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8))
    return out


def _h2v1(p):
    """(rows, n) -> (rows, 2 n): libjpeg's h2v1 fancy upsampling (plain replication for n <= 2)."""
    p = p.astype(np.int32)
    n = p.shape[1]
    if n <= 2:
        return np.repeat(p, 2, axis=1)
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * n), dtype=np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def _h2v2(p):
    p = p.astype(np.int32)
    rows, n = p.shape
    if n <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    out = np.empty((2 * rows, 2 * n), dtype=np.int32)
    for parity, far in ((0, above), (1, below)):
        s = 3 * p + far
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        o = np.empty((rows, 2 * n), dtype=np.int32)
        o[:, 0::2] = (3 * s + left + 8) >> 4
        o[:, 1::2] = (3 * s + right + 7) >> 4
        o[:, 0] = (4 * s[:, 0] + 8) >> 4
        o[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[parity::2] = o
    return out


def planes_to_rgb(planes, info):
    H, W = info["height"], info["width"]
    Y = planes[0][:H, :W].astype(np.int32)
    if info["components"] == 1:
        return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8)
    h0, v0 = info["sampling"][0]
    cw, ch = -(-W // h0), -(-H // v0)
    chroma = []
    for p in planes[1:]:
        p = p[:ch, :cw]                                   # the real downsampled extent: the MCU padding is no neighbour
        if (h0, v0) == (2, 1):
            p = _h2v1(p)
        elif (h0, v0) == (2, 2):
            p = _h2v2(p)
        chroma.append(p[:H, :W].astype(np.int32) - 128)
    cb, cr = chroma
    r = Y + ((91881 * cr + 32768) >> 16)
    b = Y + ((116130 * cb + 32768) >> 16)
    g = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data: bytes):
    """(coefficient planes, RGB image)."""
    info = parse(data)
    coefs = decode_coefficients(data, info)
    return coefs, planes_to_rgb(idct_planes(coefs, info), info)


def coefficient_checksum(coefs) -> int:
    """The checksum the stand-alone host decoder prints: FNV-1a (64 bit) over the int16 coefficients, component after component."""
    h = 0xCBF29CE484222325
    for p in coefs:
        for b in p.astype("<i2").tobytes():
            h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- test streams -----------------------------------------------------------------------------------------------------------------------
def content(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "smooth":
        a = np.stack([128 + 100 * np.sin(xx / 7.0 + 0.3) * np.cos(yy / 5.0), 128 + 90 * np.cos(xx / 11.0 - yy / 9.0), 40 + 2.5 * xx + 1.5 * yy], axis=2)
    elif kind == "noise":
        a = rng.randint(0, 256, size=(H, W, 3))
    elif kind == "checker":
        a = np.repeat((((xx + yy) & 1) * 255)[:, :, None], 3, axis=2) ^ np.array([0, 255, 0])
    elif kind == "saturated":
        a = rng.randint(0, 2, size=(H, W, 3)) * 255
    else:
        raise ValueError(kind)
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(arr: np.ndarray, quality: int = 75, subsampling=0, optimize: bool = False, restart_blocks: int = 0, gray: bool = False, **kw) -> bytes:
    import io

    from PIL import Image

    img = Image.fromarray(arr[:, :, 0] if gray else arr)
    buf = io.BytesIO()
    args = dict(quality=quality, optimize=optimize, **kw)
    if not gray:
        args["subsampling"] = subsampling
    if restart_blocks:
        args["restart_marker_blocks"] = restart_blocks
    img.save(buf, "JPEG", **args)
    return buf.getvalue()


def pil_rgb(data: bytes) -> np.ndarray:
    import io

    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def widen_dqt(data: bytes, scale: int = 3) -> bytes:
    """The same file with every quantisation table rewritten at 16-bit precision, its values multiplied by `scale` (Pillow's encoder
    never writes 16-bit tables; its decoder reads them)."""
    out, pos = bytearray(data[:2]), 2
    while True:
        assert data[pos] == 0xFF
        m, n = data[pos + 1], (data[pos + 2] << 8) | data[pos + 3]
        seg = data[pos + 4: pos + 2 + n]
        if m == 0xDB:
            body, k = bytearray(), 0
            while k < len(seg):
                assert seg[k] >> 4 == 0
                body.append(0x10 | (seg[k] & 15))
                for v in seg[k + 1: k + 65]:
                    body += int(v * scale).to_bytes(2, "big")
                k += 65
            out += bytes([0xFF, 0xDB]) + (len(body) + 2).to_bytes(2, "big") + body
        else:
            out += data[pos: pos + 2 + n]
        pos += 2 + n
        if m == 0xDA:
            return bytes(out) + data[pos:]


SMALL_SIZES = [(1, 1), (8, 8), (17, 33), (29, 37), (50, 31)]


def full_grid(H: int, W: int):
    """(id, bytes) for every combination at one size: subsampling 0 / 1 / 2 / grayscale x quality 5 / 30 / 75 / 100 x optimised or
    standard tables x restart_marker_blocks 0 / 2 x four kinds of content = 256 streams."""
    import itertools

    out = []
    for n, (sub, q, opt, rst, kind) in enumerate(itertools.product((0, 1, 2, "gray"), (5, 30, 75, 100), (False, True), (0, 2),
                                                                   ("smooth", "noise", "checker", "saturated"))):
        data = encode(content(kind, H, W, n), q, 0 if sub == "gray" else sub, opt, rst, gray=sub == "gray")
        out.append((f"{H}x{W} sub={sub} q={q} optimize={opt} restart={rst} {kind}", data))
    return out


def small_grid():
    """(id, bytes) over the small sizes: every subsampling and grayscale, qualities 5 / 30 / 75 / 100, optimised and standard tables, with
    and without restart markers, four kinds of content -- each size meets every value of every axis (not the full product)."""
    kinds = ["smooth", "noise", "checker", "saturated"]
    quals = [5, 30, 75, 100]
    out = []
    for si, (H, W) in enumerate(SMALL_SIZES):
        for j, sub in enumerate([0, 1, 2, "gray"]):
            for k in range(4):
                kind, q = kinds[(j + k + si) % 4], quals[k]
                opt, rst = bool((j + k) & 1), 2 if ((j + k + si) >> 1) & 1 else 0
                arr = content(kind, H, W, seed=si * 16 + j * 4 + k)
                data = encode(arr, q, 0 if sub == "gray" else sub, opt, rst, gray=sub == "gray")
                out.append((f"{H}x{W}-{sub}-q{q}-{kind}-{'opt' if opt else 'std'}-rst{rst}", data))
    return out
