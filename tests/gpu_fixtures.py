"""Shared helpers for the GPU parity tests: build product GPs from the golden fixtures; device copies, bit comparisons
and the library's transform-route switch for the stage-by-stage tests."""
import os

import numpy as np
import torch

import fastgaussianprocesses_amd as F

DEV = "cuda"


def product_gp(g, **kw):
    fam = str(g["family"])
    d = int(g["d"])
    B = int(g["B"])
    extra = dict(kw)
    if B > 0:
        extra["shape_batch"] = [B]
    if bool(g["per_output"]):
        extra["shape_scale"] = [B, 1]
        extra["shape_lengthscales"] = [B, d]
    if fam == "lattice":
        seq = F.Lattice(d, randomize="SHIFT", generating_vector=g["z"], shift=g["shift"])
        gp = F.FastGPLattice(seq, alpha=int(g["alpha"]), device=DEV, **extra)
    else:
        seq = F.DigitalNetB2(d, randomize="DS", generating_matrices=g["C"].astype(np.uint64), t=int(g["t"]),
                             shift=g["shift"].astype(np.uint64))
        gp = F.FastGPDigitalNetB2(seq, alpha=int(g["alpha"]), device=DEV, **extra)
    n = 2 ** int(g["m"])
    x = gp.get_x_next(n)
    assert np.array_equal(x.cpu().numpy(), g["x"]), "point generation differs from the reference fixture"
    gp.add_y_next(torch.from_numpy(g["y"]).to(DEV))
    return gp


def rel_err(a, b):
    a = torch.as_tensor(a).detach().cpu().reshape(-1)
    b = (b.detach().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b))).reshape(-1)
    if b.numel() == 0:
        return 0.0
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


def abs_err(a, b):
    a = torch.as_tensor(a).detach().cpu().reshape(-1)
    b = (b.detach().cpu() if torch.is_tensor(b) else torch.as_tensor(np.asarray(b))).reshape(-1)
    return float((a - b).abs().max()) if b.numel() else 0.0


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def to_np(t):
    return t.cpu().numpy().copy()


def raw_stream():
    from fastgaussianprocesses_amd import _native as N
    return N.stream_ptr(torch.device(DEV, torch.cuda.current_device()))


def bits(t):
    """The bytes of a tensor of any dtype and stride, as a flat uint8 tensor."""
    return torch.empty(t.numel(), dtype=t.dtype, device=t.device).copy_(t.reshape(-1)).view(torch.uint8)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def uses_r2c(lattice, log2n):
    """use_r2c(read_switches(), ...) of csrc/fgp_runtime.h: the half-length lattice transforms from n = 2^17 unless
    FGP_R2C starts with '0' (the library reads the same variable at every call)."""
    return bool(lattice) and log2n >= 17 and os.environ.get("FGP_R2C", "")[:1] != "0"
