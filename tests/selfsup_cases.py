"""Seeded inputs and the call helpers of the self-supervised criterion's tests.  Not collected; imported by
tests/test_selfsup_host.py and tests/test_hip_selfsup.py.

The shapes are the smallest at which the kernel can go wrong: 6 x 10 (less than one wave), 33 x 70 (odd, rows that are no multiple
of a wave, several passes of a workgroup over one chunk), 32 x 64 (rows of exactly one wave) and 5 x 130 (a row end two pixels past
two waves).  A thread owns one pixel and a chunk is a stretch of consecutive pixels that starts and ends anywhere in a row."""
import ctypes
import functools

import numpy as np
import torch

import selfsup_ref as sr

SHAPES = ((6, 10), (33, 70), (32, 64), (5, 130))
KINK_CAP = 0.01                    # the share of gradient elements that may sit on a kink of the sampler


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_selfsup.so (built on demand)."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_selfsup()
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n != "pf_selfsup_loss_batch"))
    lib._dll.pf_emu_selfsup_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_selfsup_order.restype = None
    return lib


def _t(a, device):
    return None if a is None else torch.from_numpy(np.array(a)).to(device)


def weight(H, W):
    from prior_flow_amd.evaluate import spherical_mask
    return np.ascontiguousarray(spherical_mask(H, W), np.float32).reshape(-1)


@functools.lru_cache(maxsize=None)
def images(B, H, W, seed=0):
    """(image1, image2) fp32 [B,3,H,W] in 0..255: a few sinusoids with integer horizontal frequencies (they wrap), one sharp
    vertical bar (an edge that does not sit on the seam, where it would switch the seam pair off) and one sharp horizontal edge;
    image2 is another draw of the same family."""
    rng = np.random.default_rng(100 + seed)
    Y, X = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    out = []
    for _ in range(2):
        img = np.zeros((B, 3, H, W))
        for b in range(B):
            for c in range(3):
                a = 110 + 20 * rng.random()
                for _k in range(3):
                    kx, ky = int(rng.integers(1, 4)), rng.integers(0, 3)
                    a = a + 25 * rng.random() * np.sin(2 * np.pi * (kx * X + 0.5 * ky * Y) + 6.28 * rng.random())
                a = a + 40 * ((X >= 0.55) & (X < 0.8)) * (0.5 + rng.random()) - 35 * (Y >= 0.4) * (0.5 + rng.random())
                img[b, c] = a
        out.append(np.ascontiguousarray(np.clip(img, 0, 255), np.float32))
    for o in out:
        o.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def flows(B, n, H, W, seed=0, variant="plain"):
    """n seeded predictions fp32 [B,2,H,W], up to +-6 px.  variant "far": a twentieth of the end points past a pole and a seeded half of
    the u at +-(W - 1)."""
    rng = np.random.default_rng(200 + seed)
    out = []
    for _ in range(n):
        f = rng.uniform(-6, 6, (B, 2, H, W))
        if variant == "far":
            pole = rng.random((B, H, W)) < 0.05
            f[:, 1][pole] = np.where(rng.random(int(pole.sum())) < 0.5, -(H + 3.5), H + 2.25)
            wide = rng.random((B, H, W)) < 0.5
            f[:, 0][wide] = np.where(rng.random(int(wide.sum())) < 0.5, -(W - 1.0), W - 1.0)
        f = np.ascontiguousarray(f, np.float32)
        f.setflags(write=False)
        out.append(f)
    return tuple(out)


def mask_of(B, H, W, seed=0, share=0.15):
    return (np.random.default_rng(300 + seed).random((B, H, W)) < share).astype(np.uint8)


def gamma_weights(n, gamma=0.8):
    return [gamma ** (n - i - 1) for i in range(n)]


def call(lib, preds, image1, image2, w, mask, i_weights, prm=sr.Params(), nblk=3, device="cpu", blocks=0, want_grads=True,
         grads=None, partials=None):
    """One raw pf_selfsup_loss_batch through `lib` (the emulation on the cpu, the product's handle on the device).  Returns (grads:
    list of numpy [B,2,H,W] or None, partials numpy [n,B,nblk,4]).  grads / partials: tensors to write into (else fresh, filled
    with NaN so that an element left unwritten shows)."""
    B, _, H, W = image1.shape
    n = len(preds)
    tp = [_t(p, device) for p in preds]
    if grads is None and want_grads:
        grads = [torch.full((B, 2, H, W), float("nan"), device=device) for _ in range(n)]
    if partials is None:
        partials = torch.full((n, B, nblk, 4), float("nan"), dtype=torch.float64, device=device)
    lib.selfsup_loss_batch(tp, _t(image1, device), _t(image2, device), _t(w, device), _t(mask, device), i_weights, grads, partials,
                           sr.z_of(w, B), prm.w_photo, prm.w_smooth, prm.eps_photo, prm.eps_smooth, prm.edge_lambda, prm.max_flow,
                           blocks=blocks)
    if device != "cpu":
        torch.cuda.synchronize()
    return (None if grads is None else [None if g is None else g.cpu().numpy() for g in grads]), partials.cpu().numpy()


def check(got_grads, got_part, ref, what, scale=1.0):
    """Losses, partial sums and every gradient element of one call against the restatement's terms `ref` (selfsup_ref.criterion)
    within `scale` times the bounds.  Elements of a pixel whose sampling fraction lies within its bound of an integer may differ:
    they are counted and capped at KINK_CAP.  Returns the worst error / bound."""
    worst = 0.0
    tot = got_part.sum(axis=(1, 2))
    for i, t in enumerate(ref):
        assert np.isfinite(got_part[i]).all(), (what, i)
        for j, key, bound in ((0, "photo", t["e_photo"]), (1, "smooth", t["e_smooth"]), (2, "used", sr.OPS * t["used"])):
            err = abs(tot[i, j] - t[key])
            assert err <= scale * bound + 1e-300, (what, i, key, err, bound)
            worst = max(worst, err / max(bound, 1e-300) / scale)
        assert tot[i, 3] == t["left_out"], (what, i, tot[i, 3], t["left_out"])
        if got_grads is None or got_grads[i] is None:
            continue
        g = got_grads[i]
        assert np.isfinite(g).all(), (what, i, "a gradient element is not finite or was not written")
        free = np.broadcast_to(t["near"][:, None], g.shape)
        assert free.mean() <= KINK_CAP, (what, i, free.mean())
        err = np.abs(g - t["grads"])
        bound = scale * t["e_grads"]
        bad = (err > bound) & ~free
        assert not bad.any(), (what, i, int(bad.sum()), float((err / np.maximum(bound, 1e-300))[~free].max()))
        if (~free).any():
            nz = ~free & (t["e_grads"] > 0)
            if nz.any():
                worst = max(worst, float((err[nz] / bound[nz]).max()))
            assert not err[~free & (t["e_grads"] == 0)].any(), (what, i, "non-zero where the statement is exactly zero")
    return worst
