"""Guard bands around device buffers: a kernel that writes or reads outside the buffers it was handed fails a test.

The parity tests look at output tensors only.  An overrun past an output, a workspace query that reports less than its kernels
index, a read past an input and a write into an input all land in whatever the caching allocator placed next to the buffer and go
unseen.  Here every buffer a kernel gets is a window into one uint8 allocation

    [ front guard | payload | tail guard ]

  * the payload starts at a 256-byte-aligned address (asserted) and the tail guard at the very next byte after the last payload
    element -- nothing is rounded up, so an overrun of one element is seen;
  * the guard size is a condition, not a measurement: the larger of 64 KiB and 256 rows of the tensor (256 * ld * itemsize, the
    tallest tile in the library), rounded up to 4096 bytes, the same on both sides.  ld is the last dimension of a tensor of two or
    more dimensions and one element otherwise (`ld=` overrides it);
  * role "out":   payload 0xFF bytes (NaN as fp32, bf16 and fp16: a skipped write shows), guards 0xA5;
  * role "in":    payload = init, guards 0xFF: a read past either end that enters the arithmetic turns an output non-finite;
                  verify() also requires the payload to be byte-identical to init (no kernel scribbles on an input);
  * role "inout": as "in", for buffers a kernel updates in place (optimizer state, the sampler's x): the payload is the caller's to
                  compare;
  * role "ws":    payload of exactly the byte count asked for (no max(n, 256), no rounding), 0xFF; guards 0xA5.

verify() compares on the device the tensor lives on, after a synchronize; a mismatch names the first and last offending byte offset
relative to the payload edge (negative: in front of the payload; >= 0 behind its end).

Plain module (not a conftest): the tests import it like numerics.py and helpers.py.  It works on CPU tensors too
(test_guards_cpu.py).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch

ALIGN = 256
MIN_GUARD = 64 << 10
GUARD_ROWS = 256
PAGE = 4096
FILL_OUT_GUARD = 0xA5
FILL_NAN = 0xFF
ROLES = ("out", "in", "inout", "ws")


def guard_bytes(ld: int, itemsize: int) -> int:
    """max(64 KiB, 256 rows of ld elements), rounded up to 4096 bytes."""
    n = max(MIN_GUARD, GUARD_ROWS * int(ld) * int(itemsize))
    return (n + PAGE - 1) // PAGE * PAGE


class GuardedTensor:
    def __init__(self, shape, dtype, device, role: str, init: Optional[torch.Tensor] = None, ld: Optional[int] = None, name: str = ""):
        if role not in ROLES:
            raise ValueError(f"role {role!r}: one of {ROLES}")
        shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        if role == "ws":
            dtype = torch.uint8
            if len(shape) != 1:
                raise ValueError("a workspace is a byte count")
        if role in ("in", "inout"):
            if init is None:
                raise ValueError(f"role {role!r} needs init")
            if tuple(init.shape) != shape or init.dtype != dtype:
                raise ValueError(f"init {tuple(init.shape)} {init.dtype} does not match {shape} {dtype}")
        elif init is not None:
            raise ValueError(f"role {role!r} takes no init")
        self.role, self.shape, self.dtype, self.name = role, shape, dtype, name or role
        itemsize = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        self.nbytes = numel * itemsize
        if ld is None:
            ld = shape[-1] if len(shape) >= 2 else 1
        self.guard = guard_bytes(max(1, ld), itemsize)
        self.buf = torch.empty(self.guard + ALIGN + self.nbytes + self.guard, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = self.guard + (-(base + self.guard)) % ALIGN      # payload offset inside buf
        self.end = self.start + self.nbytes                           # first byte of the tail guard
        self.ptr = base + self.start                                  # (data_ptr() of an EMPTY view is 0: use this)
        assert self.ptr % ALIGN == 0, f"{self.name}: payload at {self.ptr:#x} is not {ALIGN}-byte aligned"
        assert self.end + self.guard <= self.buf.numel()
        self.guard_fill = FILL_NAN if role in ("in", "inout") else FILL_OUT_GUARD
        self.buf.fill_(self.guard_fill)
        self.payload = self.buf[self.start:self.end].view(dtype).view(shape)
        assert numel == 0 or self.payload.data_ptr() == self.ptr
        self._init_bytes = None
        if init is not None:
            self.payload.copy_(init)
            self._init_bytes = self.payload_bytes().clone()
        else:
            self.payload_bytes().fill_(FILL_NAN)

    # ---- views ---------------------------------------------------------------------------------------------------------------------------
    def payload_bytes(self) -> torch.Tensor:
        return self.buf[self.start:self.end]

    def front_guard(self) -> torch.Tensor:
        return self.buf[self.start - self.guard:self.start]

    def tail_guard(self) -> torch.Tensor:
        return self.buf[self.end:self.end + self.guard]

    def data_ptr(self) -> int:
        return self.ptr

    # ---- checks --------------------------------------------------------------------------------------------------------------------------
    def problems(self) -> List[str]:
        """Every violation as one line (empty: clean).  The caller synchronises first."""
        out = []
        for side, g, origin in (("front", self.front_guard(), -self.guard), ("tail", self.tail_guard(), 0)):
            bad = g != self.guard_fill
            if bool(bad.any()):
                idx = bad.nonzero().flatten()
                first, last = int(idx[0]) + origin, int(idx[-1]) + origin
                edge = "payload start" if side == "front" else "payload end"
                out.append(f"{self.name} ({self.role}, {self.shape} {self.dtype}, guard {self.guard} B): {int(bad.sum())} bytes of the {side} "
                           f"guard changed, offsets {first} .. {last} relative to the {edge}")
        if self.role == "in":
            bad = self.payload_bytes() != self._init_bytes
            if bool(bad.any()):
                idx = bad.nonzero().flatten()
                out.append(f"{self.name} (in, {self.shape} {self.dtype}): the input payload changed in {int(bad.sum())} bytes, "
                           f"offsets {int(idx[0])} .. {int(idx[-1])} relative to the payload start")
        return out

    def verify(self) -> None:
        _verify([self], self.buf.device)


def _verify(items, device) -> None:
    """synchronise once, then assert that none of `items` reports a problem"""
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    p = [line for t in items for line in t.problems()]
    assert not p, "\n".join(p)


def guarded(shape, dtype, device, role: str, init: Optional[torch.Tensor] = None, ld: Optional[int] = None, name: str = "") -> GuardedTensor:
    return GuardedTensor(shape, dtype, device, role, init=init, ld=ld, name=name)


class Guards:
    """The guarded tensors of one case: ``g = Guards(device)``, ``g.inp(t)``, ``g.out(shape, dtype)``, ``g.ws(nbytes)`` ..., then one
    ``g.verify_all()``.  Also a context manager: leaving the block without an exception verifies."""

    def __init__(self, device):
        self.device = device
        self.items: List[GuardedTensor] = []

    def _add(self, t: GuardedTensor) -> GuardedTensor:
        self.items.append(t)
        return t

    def out(self, shape, dtype=torch.float32, name: str = "", ld: Optional[int] = None) -> GuardedTensor:
        return self._add(GuardedTensor(shape, dtype, self.device, "out", ld=ld, name=name or f"out{len(self.items)}"))

    def inp(self, init: torch.Tensor, name: str = "", ld: Optional[int] = None) -> GuardedTensor:
        return self._add(GuardedTensor(init.shape, init.dtype, self.device, "in", init=init, ld=ld, name=name or f"in{len(self.items)}"))

    def inout(self, init: torch.Tensor, name: str = "", ld: Optional[int] = None) -> GuardedTensor:
        return self._add(GuardedTensor(init.shape, init.dtype, self.device, "inout", init=init, ld=ld, name=name or f"inout{len(self.items)}"))

    def ws(self, nbytes: int, name: str = "", ld: Optional[int] = None) -> GuardedTensor:
        return self._add(GuardedTensor((int(nbytes),), torch.uint8, self.device, "ws", ld=ld, name=name or f"ws{len(self.items)}"))

    def outputs(self) -> Sequence[GuardedTensor]:
        return [t for t in self.items if t.role == "out"]

    def verify_all(self) -> None:
        _verify(self.items, self.device)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.verify_all()
        return False
