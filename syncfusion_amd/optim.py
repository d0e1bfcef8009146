"""The optimizer stage of the reference's training step on HIP: clip-by-global-norm and AdamW in one C-ABI call.

What the reference configures (exp/train_diffusion_gh.yaml:91-92 ``gradient_clip_val: 0.5``, main/module_diffusion.py:53-62 and
main/module_onset.py: ``torch.optim.AdamW``) ran here as ``torch.nn.utils.clip_grad_norm_`` -- a per-tensor norm pass and a read-modify-write
scaling pass over every gradient -- followed by torch's fused AdamW.  ``AdamW`` below is a ``torch.optim.AdamW`` whose ``step()`` hands ONE
device-resident descriptor table of every (parameter, gradient, exp_avg, exp_avg_sq, step) to ``sf_optim_adamw_step``
(syncfusion_amd/csrc/optim.hip): a sum-of-squares pass over the gradients, one small workgroup that turns it into the clip coefficient and
advances the step counters, and the update pass, which applies the coefficient in registers.

    ``.grad`` is NOT scaled: ``clip_grad_norm_`` multiplies the gradients in place, this class leaves them as backward wrote them and uses
    ``g * clip_coef`` inside the update only.  Code that reads ``.grad`` after the step sees the unclipped values.

The state layout is torch's own (``step`` an fp32 device scalar as torch keeps it for ``fused=True``, ``exp_avg``, ``exp_avg_sq``), so
``state_dict()`` / ``load_state_dict()`` interchange with ``torch.optim.AdamW`` in both directions, and LR schedulers see a plain
``torch.optim.AdamW``.  Hyper-parameters and ``max_grad_norm`` live in a small device array the kernels read: nothing that changes per
step is a kernel argument, so the whole call can sit inside a captured graph (``training.GraphedTrainStep(..., optimizer=opt)``).
"""
from __future__ import annotations

import warnings
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib

CHUNK = 16384          # elements per chunk = per workgroup (SF_OPTIM_CHUNK in include/syncfusion_amd.h)
DESC_WORDS = 8         # 64-bit words per table record: p, g, exp_avg, exp_avg_sq, step, numel, group | first_chunk << 32, 0
HYPER_STRIDE = 8       # doubles per hyper-parameter record; record 0 holds max_norm, record 1 + g the group g


def chunks_of(numel: int) -> int:
    return (int(numel) + CHUNK - 1) // CHUNK


def build_table(records: Sequence[Tuple[int, int, int, int, int, int, int]]) -> Tuple[torch.Tensor, int]:
    """``records``: (p, g, exp_avg, exp_avg_sq, step addresses, numel, group) per tensor -> the (n, 8) int64 host table in the layout
    ``sf_optim_adamw_step`` documents, and the total chunk count."""
    rows: List[List[int]] = []
    first = 0
    for p, g, m, v, step, numel, group in records:
        if numel < 1:
            raise ValueError("empty tensors have no chunk: leave them out of the table")
        rows.append([_i64(p), _i64(g), _i64(m), _i64(v), _i64(step), int(numel), int(group) | (first << 32), 0])
        first += chunks_of(numel)
        if first >= 2 ** 31:
            raise ValueError("more than 2^31 chunks")
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), DESC_WORDS), first


def _i64(address: int) -> int:
    return address - (1 << 64) if address >= (1 << 63) else address


class AdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` (decoupled weight decay, ``amsgrad=False``, ``maximize=False``) whose step, and the global-norm clipping in
    front of it when ``max_grad_norm`` is set, run in the HIP library.  CPU, non-fp32, non-contiguous or sparse tensors and the ``amsgrad`` /
    ``maximize`` / ``capturable`` variants are handed to ``torch.optim.AdamW.step`` (after ``clip_grad_norm_`` when ``max_grad_norm`` is
    set), with one warning per instance."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None, **kwargs):
        params = list(params)
        flat = [p for g in params for p in g["params"]] if params and isinstance(params[0], dict) else \
               [p[1] if isinstance(p, tuple) else p for p in params]
        if "fused" not in kwargs and "foreach" not in kwargs and flat and all(p.is_cuda and p.is_floating_point() for p in flat):
            kwargs["fused"] = True    # what super().step() runs on a fallback, and what makes load_state_dict keep `step` on the device
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kwargs)
        self.max_grad_norm = max_grad_norm
        self.table_builds = 0           # how often the descriptor table was rebuilt (it follows the (p, g) addresses)
        self.hyper_uploads = 0
        self._key: Optional[tuple] = None
        self._table_host: Optional[torch.Tensor] = None
        self._table_dev: Optional[torch.Tensor] = None
        self._total_chunks = 0
        self._ws: Optional[torch.Tensor] = None
        self._result: Optional[torch.Tensor] = None
        self._hyper_vals: Optional[tuple] = None
        self._hyper_dev: Optional[torch.Tensor] = None
        self._pending: List[Tuple[torch.Tensor, torch.Tensor]] = []   # (device, host) copies a graph capture could not issue
        self._clipped = False
        self._warned = False

    # ---- what the step works on ---------------------------------------------------------------------------------------------------------
    def _entries(self) -> List[Tuple[torch.Tensor, int]]:
        """(parameter, group index) of every parameter that has a gradient; one without is skipped whole, as torch does."""
        return [(p, gi) for gi, group in enumerate(self.param_groups) for p in group["params"] if p.grad is not None]

    def _fallback_reason(self, entries) -> Optional[str]:
        for group in self.param_groups:
            for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
                if group.get(flag):
                    return f"{flag}=True"
            if any(isinstance(group[k], torch.Tensor) for k in ("lr", "eps", "weight_decay")) or any(isinstance(b, torch.Tensor) for b in group["betas"]):
                return "tensor hyper-parameters"
        dev = entries[0][0].device
        for p, _ in entries:
            g = p.grad
            if not p.is_cuda or p.device != dev or g.device != dev:
                return "parameters outside one GPU"
            if g.is_sparse:
                return "sparse gradients"
            if p.dtype != torch.float32 or g.dtype != torch.float32:
                return "non-fp32 parameters or gradients"
            if not p.is_contiguous() or not g.is_contiguous() or g.shape != p.shape:
                return "non-contiguous parameters or gradients"
        return None

    def _state_of(self, p: torch.Tensor) -> dict:
        """torch's lazy state (``Adam._init_group`` with fused=True): created at the parameter's first step; a ``step`` that a checkpoint of
        the unfused optimizer left on the host, or in another dtype, moves to an fp32 device scalar."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        step = st["step"]
        if not (isinstance(step, torch.Tensor) and step.device == p.device and step.dtype == torch.float32 and step.dim() == 0):
            st["step"] = (step.detach().to(device=p.device, dtype=torch.float32).reshape(()).clone() if isinstance(step, torch.Tensor)
                          else torch.tensor(float(step), dtype=torch.float32, device=p.device))
        for k in ("exp_avg", "exp_avg_sq"):
            t = st[k]
            if t.device != p.device or t.dtype != torch.float32 or not t.is_contiguous() or t.shape != p.shape:
                st[k] = t.detach().to(device=p.device, dtype=torch.float32).reshape(p.shape).contiguous()
        return st

    def _upload(self, dev: torch.Tensor, host: torch.Tensor) -> None:
        """A host-to-device copy on the current stream; while that stream is being captured the copy waits in ``_pending`` (the captured
        kernels only hold the device buffer's address) until ``sync_device_state()`` issues it after the capture."""
        if dev.is_cuda and torch.cuda.is_current_stream_capturing():
            self._pending = [(d, h) for d, h in self._pending if d is not dev] + [(dev, host)]
        else:
            dev.copy_(host)

    def sync_device_state(self) -> None:
        """Issue the copies a graph capture deferred, and upload the hyper-parameters (``lr`` .. ``weight_decay`` per group,
        ``max_grad_norm``) if any changed: call it before replaying a graph that holds this optimizer's step
        (``GraphedTrainStep.step`` does), so an LR scheduler's new value reaches the captured kernels."""
        pending, self._pending = self._pending, []
        for dev, host in pending:
            dev.copy_(host)
        if self._hyper_dev is not None:
            self._sync_hyper(self._hyper_dev.device)

    def _sync_hyper(self, device: torch.device) -> None:
        vals = [float(self.max_grad_norm) if self.max_grad_norm is not None else 0.0] + [0.0] * (HYPER_STRIDE - 1)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            vals += [float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"])] + [0.0] * (HYPER_STRIDE - 5)
        key = (str(device),) + tuple(vals)
        if key != self._hyper_vals:
            if self._hyper_dev is None or self._hyper_dev.device != device or self._hyper_dev.numel() != len(vals):
                self._hyper_dev = torch.empty(len(vals), dtype=torch.float64, device=device)
            self._upload(self._hyper_dev, torch.tensor(vals, dtype=torch.float64))
            self._hyper_vals = key
            self.hyper_uploads += 1

    def _prepare(self, entries) -> None:
        """State, descriptor table (rebuilt and uploaded only when a parameter's or a gradient's address differs from the last call's),
        hyper-parameter array, workspace.  Touches no kernel: it works on CPU tensors too (the tests of the table do that)."""
        device = entries[0][0].device
        key = (str(device),) + tuple(a for p, gi in entries for a in (p.data_ptr(), p.grad.data_ptr(), gi))
        if key != self._key:
            records = []
            for p, gi in entries:
                st = self._state_of(p)
                records.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr(),
                                p.numel(), gi))
            self._table_host, self._total_chunks = build_table(records)
            if self._table_dev is None or self._table_dev.device != device or self._table_dev.shape != self._table_host.shape:
                self._table_dev = torch.empty(self._table_host.shape, dtype=torch.int64, device=device)
            self._upload(self._table_dev, self._table_host)
            self._key = key
            self.table_builds += 1
        self._sync_hyper(device)
        if self._result is None or self._result.device != device:
            self._result = torch.zeros(2, dtype=torch.float32, device=device)

    # ---- torch.optim.Optimizer surface --------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._key = None            # the moments and step counters are new tensors: the table's addresses are stale

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """Global L2 norm of the gradients of the last clipped step: a device scalar (a view of the kernels' result buffer that the next
        step overwrites; reading it does not synchronise here).  None before the first clipped step."""
        return self._result[0] if self._clipped and self._result is not None else None

    @property
    def last_clip_coef(self) -> Optional[torch.Tensor]:
        return self._result[1] if self._result is not None else None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = [(p, gi) for p, gi in self._entries() if p.numel() > 0]
        if not entries:
            return loss
        reason = self._fallback_reason(entries)
        if reason is not None:
            if not self._warned:
                self._warned = True
                warnings.warn(f"syncfusion_amd.optim.AdamW: {reason}: this step runs torch.optim.AdamW.step (the HIP kernels take fp32 contiguous "
                              "tensors on one GPU, amsgrad / maximize / capturable off)", stacklevel=2)
            if self.max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_([p for p, _ in entries], self.max_grad_norm)
            super().step()
            return loss
        self._prepare(entries)
        device = entries[0][0].device
        lib = _lib.load()
        need = int(lib.sf_optim_workspace_bytes(self._total_chunks))
        if self._ws is None or self._ws.device != device or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=device)
        clip = 1 if self.max_grad_norm is not None else 0
        with torch.cuda.device(device):
            _lib.check(lib.sf_optim_adamw_step(self._table_dev.data_ptr(), len(entries), self._total_chunks, self._hyper_dev.data_ptr(),
                                               len(self.param_groups), clip, self._result.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                               _lib.stream_ptr(device)), "sf_optim_adamw_step")
        self._clipped = bool(clip)
        return loss
