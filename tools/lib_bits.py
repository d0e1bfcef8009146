#!/usr/bin/env python3
"""Bit identity of two builds of the HIP library on ONE Python tree (a kernel refactor must not move a bit).

    SF_LIB_PATH=<lib> [SF_...=1] python tools/lib_bits.py dump DIR GROUP[,GROUP...]     one fresh process per library
    python tools/lib_bits.py compare DIR_A DIR_B [TITLE]                                   (no GPU)

dump runs the groups' cases on fixed seeds with the library SF_LIB_PATH names and writes DIR/<case>.pt, a dict of CPU tensors (and, where
the dispatcher is asked, the kernel label as a string).  compare prints one row per case -- tensors, values, "bit-identical" or the first
tensor that differs -- comparing the raw bytes (NaN payloads and signed zeros count), and exits 1 on any difference or missing case.

Groups:
    eval-bf16 | eval-fp16 | eval-fp32 | eval-fp32x   one U-Net evaluation (a one-step sample) of that engine, 2 clips, L0 = 45056
    prenorm     sf_op_inject_prenorm_proj at (4, 44, 1024, 256, 1536) and (7, 301, 256, 64, 384), bf16 and fp16: z and q
    conv1d      sf_op_conv1d_cl on every row of tests/test_gpu_conv1d_elementwise.py that names conv_gemm_sk / _v2 / _fast / _wp / _rs
    train       one training step (loss and every gradient) of the small model of tests/test_gpu_train.py, 2 clips of 192 samples
The final sample of configs[1] is `bench.py --dump-outputs DIR`: compare reads a sample.npy in DIR as one more case."""
import ctypes as C
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch  # noqa: E402

FAMILIES = ("conv_gemm_sk<", "conv_gemm_v2<", "conv_gemm_fast<", "conv_gemm_wp<", "conv_gemm_rs<")
PRENORM = [(4, 44, 1024, 256, 1536), (7, 301, 256, 64, 384)]
TD = {"fp32": torch.float32, "fp32x": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def save(out_dir, case, tensors):
    torch.cuda.synchronize()
    torch.save({k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in tensors.items()}, os.path.join(out_dir, case + ".pt"))
    print(f"dumped {case}: {len(tensors)} entries", flush=True)


def dump_eval(out_dir, dtype, dev):
    import bench

    with torch.no_grad():
        model = bench.build_model(dtype, dev)
        nz = torch.randn(2, 1, bench.L0, generator=torch.Generator().manual_seed(1000)).to(dev)
        ch, e = bench.synthetic_conditioning(model, 2, bench.L0, dev, real=True)
        y = model.model.sample(x_noisy=nz, num_steps=1, channels=ch, embedding=e, embedding_scale=1.0)
    save(out_dir, f"eval-{dtype}", {"sample": y})


def dump_prenorm(out_dir, dev):
    from syncfusion_amd import _lib as _l

    lib = _l.load()
    for dtype in ("bf16", "fp16"):
        for (B, L, Cc, C2, N) in PRENORM:
            td = TD[dtype]
            g = torch.Generator().manual_seed(B * 1000 + L + Cc)
            m = (torch.randn(B, L, Cc, generator=g) * 1.3 + 0.4).to(td).to(dev)
            ctx = torch.randn(B, L, C2, generator=g).to(td).to(dev)
            ops = [torch.randn(Cc, Cc + C2, generator=g) / (Cc + C2) ** 0.5, torch.randn(Cc, generator=g) * 0.1, 1 + 0.2 * torch.randn(Cc, generator=g),
                   0.1 * torch.randn(Cc, generator=g), torch.randn(N, Cc, generator=g) / Cc ** 0.5]
            ops = [t.contiguous().to(dev) for t in ops]
            z = torch.full((B, L, Cc), float("nan"), dtype=td, device=dev)
            q = torch.full((B, L, N), float("nan"), dtype=td, device=dev)
            ws = torch.zeros(lib.sf_op_inject_prenorm_proj_workspace_bytes(B, L, Cc, C2, N), dtype=torch.uint8, device=dev)
            fused = C.c_int(-1)
            _l.check(lib.sf_op_inject_prenorm_proj(_l.DTYPES[dtype], m.data_ptr(), ctx.data_ptr(), ops[0].data_ptr(), ops[1].data_ptr(), ops[2].data_ptr(),
                                                   ops[3].data_ptr(), 1e-5, ops[4].data_ptr(), B, L, Cc, C2, N, z.data_ptr(), q.data_ptr(), C.byref(fused),
                                                   ws.data_ptr(), ws.numel(), _l.stream_ptr(dev)), "sf_op_inject_prenorm_proj")
            save(out_dir, f"prenorm-{dtype}-B{B}-L{L}-C{Cc}-C2{C2}-N{N}", {"z": z, "q": q, "fused": str(fused.value)})


def dump_conv1d(out_dir, dev):
    import conv1d_ref as R
    from test_gpu_conv1d_elementwise import CASES, case_id, variant

    from syncfusion_amd import _lib as _l

    lib = _l.load()
    for c in CASES:
        if not c.expected_label.startswith(FAMILIES):
            continue
        x, w, _, bias, res = R.operands(c)
        td = TD[c.dtype]
        xd, wd, bd = x.to(td).to(dev), w.to(dev), bias.to(dev)
        rd = res.to(td).to(dev) if c.residual else None
        out = torch.full((c.B, c.Lout, c.N), float("nan"), dtype=td, device=dev)
        ws = torch.zeros(16 * c.N * c.K + (1 << 20), dtype=torch.uint8, device=dev)
        label = variant(lib, _l, c)
        _l.check(lib.sf_op_conv1d_cl(_l.DTYPES[c.dtype], xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), None, None, 0, 0.0, rd.data_ptr() if c.residual else None,
                                     c.B, c.L, c.C, c.N, c.taps, c.stride, c.pad, c.up, out.data_ptr(), ws.data_ptr(), ws.numel(), _l.stream_ptr(dev)),
                 "sf_op_conv1d_cl")
        save(out_dir, "conv1d-" + case_id(c) + "-" + c.expected_label.split("<")[0][10:], {"out": out, "label": label})


def dump_train(out_dir, dev):
    from test_gpu_train import _small_training_model

    m = _small_training_model(dev)
    B, L0 = 2, 16 * 12
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, 1, L0, generator=g).to(dev)
    y = (torch.rand(B, 1, L0, generator=g) < 0.03).float().to(dev)
    torch.manual_seed(1000)
    loss = m.training_step((x, y, x, None, None), 0)
    loss.backward()
    t = {"loss": loss}
    t.update({"grad:" + n: p.grad for n, p in m.named_parameters() if p.grad is not None})
    save(out_dir, "train-step", t)


def dump(out_dir, groups):
    os.makedirs(out_dir, exist_ok=True)
    dev = torch.device("cuda", 0)
    for gname in groups:
        if gname.startswith("eval-"):
            dump_eval(out_dir, gname[5:], dev)
        else:
            {"prenorm": dump_prenorm, "conv1d": dump_conv1d, "train": dump_train}[gname](out_dir, dev)
    return 0


def raw(t):
    return t.contiguous().view(-1).view(torch.uint8)


def load_case(path):
    if path.endswith(".npy"):
        import numpy as np

        return {"sample": torch.from_numpy(np.load(path))}
    return torch.load(path)


def compare(dir_a, dir_b, title=None):
    names = sorted({os.path.basename(p) for d in (dir_a, dir_b) for p in glob.glob(os.path.join(d, "*.pt")) + glob.glob(os.path.join(d, "*.npy"))})
    if title:
        print(title)
    print(f"{'case':78s} {'tensors':>7s} {'values':>10s}  result")
    bad = 0 if names else 1
    for n in names:
        pa, pb = os.path.join(dir_a, n), os.path.join(dir_b, n)
        case = n.rsplit(".", 1)[0] if n != "sample.npy" else "configs[1] final sample (bench.py --dump-outputs)"
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{case:78s} {'-':>7s} {'-':>10s}  MISSING in {dir_b if os.path.exists(pa) else dir_a}")
            bad += 1
            continue
        a, b = load_case(pa), load_case(pb)
        tens = [k for k in a if torch.is_tensor(a[k])]
        note = " ".join(f"{k}={a[k]}" for k in a if not torch.is_tensor(a[k]))
        diff = [k for k in a if k not in b or (torch.is_tensor(a[k]) and (a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not torch.equal(raw(a[k]), raw(b[k]))))
                or (not torch.is_tensor(a[k]) and a[k] != b[k])] + [k for k in b if k not in a]
        vals = sum(a[k].numel() for k in tens)
        print(f"{case:78s} {len(tens):7d} {vals:10d}  {'bit-identical' if not diff else 'DIFFERS: ' + ', '.join(diff[:4])}{'   ' + note if note else ''}")
        bad += bool(diff)
    return 1 if bad else 0


def main(argv):
    if len(argv) >= 3 and argv[0] == "dump":
        return dump(argv[1], argv[2].split(","))
    if len(argv) >= 3 and argv[0] == "compare":
        return compare(argv[1], argv[2], argv[3] if len(argv) > 3 else None)
    print(__doc__)
    return 2


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
