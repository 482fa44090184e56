"""Runners shared by tests/test_splat_host.py (the host emulation) and tests/test_hip_splat.py (the device): the emulation's handle,
one call of pf_splat_accumulate + pf_splat_resolve through the typed wrappers on numpy inputs, and a case of the sweep held to
the float64 restatement (tests/splat_ref.py)."""
import ctypes
import functools

import numpy as np
import torch

import splat_ref as sr


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_splat.so (built on demand): only the three splat entry points are present."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_splat()
    keep = ("pf_splat_scratch_bytes", "pf_splat_accumulate", "pf_splat_resolve")
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in keep))
    lib._dll.pf_emu_splat_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_splat_order.restype = None
    lib._dll.pf_emu_splat_scales.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.POINTER(ctypes.c_int)]
    lib._dll.pf_emu_splat_scales.restype = None
    return lib


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def to_device(jobs, device="cpu"):
    """The jobs of splat_ref.inputs as the tuples PfLib.splat_accumulate takes (tensors on `device`)."""
    return [(_t(q["src"], device), _t(q["flow"], device), _t(q["metric"], device), _t(q["mask"], device), q["tau"], q["beta"])
            for q in jobs]


def run(lib, jobs, alpha, device="cpu", fill=None, fill_t=0.0, zmax=sr.ZMAX, vmax=sr.VMAX, cmin=sr.CMIN, resolve_vmax=None,
        tjobs=None, acc=None):
    """One call: (out [B,C,H,W] float32, hole [B,H,W] uint8, raw sums before resolve [B,C+2,H,W] int64, sums after) as numpy.
    fill: (fill0, fill1) numpy maps or None.  out and hole are filled with NaN / 255 beforehand.  tjobs: the jobs already on the
    device; acc: the sums to use (default: fresh zeros)."""
    tj = to_device(jobs, device) if tjobs is None else tjobs
    B, C, H, W = tj[0][0].shape
    if acc is None:
        acc = torch.zeros(B, C + 2, H, W, dtype=torch.int64, device=device)
    out = torch.full((B, C, H, W), float("nan"), dtype=torch.float32, device=device)
    hole = torch.full((B, H, W), 255, dtype=torch.uint8, device=device)
    f0, f1 = (None, None) if fill is None else (_t(fill[0], device), _t(fill[1], device))
    lib.splat_accumulate(tj, acc, alpha, zmax, vmax)
    raw = acc.cpu().numpy().copy()
    lib.splat_resolve(acc, out, hole, len(tj), vmax if resolve_vmax is None else resolve_vmax, cmin, f0, f1, fill_t)
    return out.cpu().numpy(), hole.cpu().numpy(), raw, acc.cpu().numpy()


DEVICE_PATHS = sr.device_paths()            # the cases for pf_splat_acc_kernel's window, beside the sweep (splat_ref.py)


def case_inputs(kind, shape, t, alpha, C, njobs):
    B, H, W = shape
    make = sr.inputs if kind in sr.FAMILIES else sr.device_inputs
    return make(kind, B, H, W, C, njobs, t, with_metric=alpha > 0)


def reached(case):
    """The window's paths (tests/launch_paths.py) that the jobs of a case reach."""
    import launch_paths as lp
    return lp.splat_case_paths(case_inputs(*case), *case[1][1:])


def check_case(lib, kind, shape, t, alpha, C, njobs, device="cpu", refs=None):
    """One case of the sweep against the float64 restatement, with the blend fill on the two-job cases; returns (out, hole, raw,
    figures per image).  refs: a dict that keeps the references of a case for the next caller."""
    B, H, W = shape
    jobs = case_inputs(kind, shape, t, alpha, C, njobs)
    fill = (jobs[0]["src"], jobs[1]["src"]) if njobs == 2 else None
    out, hole, raw, after = run(lib, jobs, alpha, device, fill, t if fill else 0.0)
    assert not after.any(), "the sums are not all-zero after the call"
    assert int(hole.max()) <= 1
    figs = []
    for b in range(B):
        key = (kind, shape, t, alpha, C, njobs, b)
        ref = refs.get(key) if refs is not None else None
        if ref is None:
            ref = sr.reference(jobs, b, alpha)
            if refs is not None:
                refs[key] = ref
        fl = None if fill is None else sr.fill_blend(fill[0][b], fill[1][b], t)
        figs.append(sr.check(out[b], hole[b], ref, fl, f"{kind} {H}x{W} t={t} alpha={alpha} C={C} jobs={njobs} image {b}"))
    return out, hole, raw, figs
