"""The stand-alone host build of the JPEG decoder's shared code (tests/jpeg_host_decode.cpp) and the deterministic corruptions the JPEG
tests feed it: compiled with ``-fsanitize=address,undefined`` and run as a child process on the CPU.  Plain module (not a conftest)."""
from __future__ import annotations

import os
import shutil
import subprocess
from typing import List, Sequence, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))


def build(out_dir: str) -> str:
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(out_dir), "jpeg_host_decode")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(HERE, "jpeg_host_decode.cpp")], check=True)
    return exe


def run(exe: str, out_dir: str, blobs: Sequence[bytes], tag: str = "f") -> List[Tuple[str, int]]:
    """One child process over all `blobs`: [(status, checksum)] per file.  Asserts exit status 0 and no sanitizer report."""
    paths = []
    for i, b in enumerate(blobs):
        p = os.path.join(str(out_dir), f"{tag}{i}.jpg")
        with open(p, "wb") as f:
            f.write(b)
        paths.append(p)
    out = []
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    for k in range(0, len(paths), 512):
        r = subprocess.run([exe] + paths[k: k + 512], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
        for line in r.stdout.splitlines():
            st, h = line.split()
            out.append((st, int(h, 16)))
    assert len(out) == len(blobs)
    return out


def truncations(data: bytes, step: int = 7) -> List[bytes]:
    return [data[:n] for n in range(0, len(data), step)]


def byte_flips(data: bytes, count: int, seed: int, lo: int = 0, hi: int = None) -> List[bytes]:
    """`count` copies of `data`, each with one byte of [lo, hi) replaced; position and value from a fixed LCG."""
    hi = len(data) if hi is None else hi
    out, x = [], seed & 0xFFFFFFFF
    for _ in range(count):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        pos = lo + (x >> 8) % (hi - lo)
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        b = bytearray(data)
        b[pos] = (b[pos] ^ (1 + (x >> 16) % 255)) & 0xFF
        out.append(bytes(b))
    return out


def plain_flips(data: bytes, count: int, seed: int) -> List[bytes]:
    """Byte flips inside the entropy-coded data that neither make nor break an FF pair (the flipped byte, its new value and the byte
    in front of it are not FF), so the stream keeps its header, its size and its markers: what jpeg_ref.entropy_status restates."""
    import jpeg_ref as R

    lo, hi = R.parse(data)["data_range"]
    out = []
    for cand in byte_flips(data, 8 * count, seed, lo, hi):
        k = next(i for i in range(len(data)) if cand[i] != data[i])
        if data[k] != 0xFF and cand[k] != 0xFF and data[k - 1] != 0xFF:
            out.append(cand)
        if len(out) == count:
            break
    assert len(out) == count
    return out


def device_corruption_batch():
    """The fixed batch of the device corruption tests: [good A, A truncated in the middle of its entropy-coded data, good B, B with the
    first plain byte flip (seed 99) that jpeg_ref.entropy_status flags].  A has restart markers, B is one segment, so B's status word is
    one definite code.  Returns (blobs, status of the flipped stream).  test_jpeg_cpu.py runs these very streams through the host build
    under ASan + UBSan; the device tests build nothing."""
    import jpeg_ref as R

    a = R.encode(R.content("noise", 17, 33, 1), 75, 2, True, 2)
    b = R.encode(R.content("smooth", 17, 33, 2), 90, 2, False, 0)
    begin, end = R.parse(a)["data_range"]
    truncated = a[: begin + (end - begin) // 2]
    flipped, code = next((f, c) for f in plain_flips(b, 32, 99) for c in [R.entropy_status(f)] if c)
    return [a, truncated, b, flipped], code


def corruption_streams():
    """Three small streams (4:2:0 optimised with restart markers, 4:4:4 standard tables, grayscale) for the corruption runs."""
    import jpeg_ref as R

    return [R.encode(R.content("noise", 17, 33, 1), 75, 2, True, 2), R.encode(R.content("smooth", 29, 37, 2), 30, 0, False, 0),
            R.encode(R.content("checker", 8, 8, 3), 95, 0, False, 0, gray=True)]
