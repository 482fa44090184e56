"""Seeded inputs and runners shared by tests/test_reproject_host.py (the host emulation) and tests/test_hip_reproject.py (the device):
the emulation's handle, projections / z-splats / updates through the typed wrappers on numpy inputs, the sweep of staged inputs
and the analytic scenes of reproject_ref with their camera paths."""
import ctypes
import functools

import numpy as np
import torch

import egomotion_cases as ec
import egomotion_ref as er
import odometry_cases as oc
import reproject_ref as rr

ENTRIES = oc.ENTRIES + ("pf_reproj_project", "pf_zsplat_bytes", "pf_zsplat_front", "pf_zsplat_accumulate", "pf_zsplat_resolve",
                        "pf_depth_update")
_t = ec._t
bits = oc.bits
# (B, C, H, W) of the sweep: every shape, B = 1..3 and C = 0, 1, 3, 4 occur; 17x37 and 33x70 take the element form
SWEEP = ((1, 0, 6, 10), (2, 1, 17, 37), (3, 3, 24, 48), (1, 4, 33, 70), (2, 3, 64, 128), (2, 1, 40, 1100))
FAMILIES = ("seam", "pole", "collapse", "two_layers", "blend", "passthrough", "junk")
TRUTH_SHAPES = ((32, 64), (48, 96))
# The share of target pixels that may stay empty on the truth scenes.  A target whose used taps (b_k >= b_min = 0.25) sum to less
# than cmin = 0.5 is a hole; for sub-pixel offsets spread evenly over the unit square that is 4.65 % of the offsets (the area
# where the largest bilinear weight is below 1/2 and no second one reaches 1/4, integrated numerically).  Flows below a pixel do not
# spread the offsets evenly, so the cap is three times that share.
HOLE_CAP = 0.14
FILTER_SIGMA = 0.15        # the noise of a measurement, as a standard deviation of log2
# how far above the restatement's ratio the emulation and the device may end: the restatement's own ratios over three seeds lie
# within a factor 1.07 of each other (test_filter_has_a_point prints and asserts it)
FILTER_FACTOR = 1.1


@functools.lru_cache(maxsize=None)
def emu():
    """PfLib handle of tests/emu/libpf_emu_reproject.so (built on demand): the depth-propagation entry points and everything an
    Odometry needs."""
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    so = ge.build_emu_reproject()
    lib = _lib.PfLib(so, require_cuda=False, optional=tuple(n for n in _lib.EXPORTS if n not in ENTRIES))
    lib._dll.pf_emu_odo_order.argtypes = [ctypes.c_ulonglong]
    lib._dll.pf_emu_odo_order.restype = None
    return lib


# ---- staged inputs of the z-splat --------------------------------------------------------------------------------------------
def staged(family, B, C, H, W, seed=0):
    """(src [B,C,H,W] or None, flow [B,2,H,W], d, weight [B,H,W] fp32, valid uint8 [B,H,W], note): the stored inputs of a z-splat."""
    rng = np.random.default_rng(seed * 101 + H * 7 + W)
    f32 = np.float32
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    flow = rng.uniform(-1.5, 1.5, (B, 2, H, W)).astype(f32)
    d = np.exp2(rng.uniform(-3, 1, (B, H, W))).astype(f32)
    weight = (rng.integers(1, 160, (B, H, W)) / 16).astype(f32)           # up to 10: some above w_max = 8
    valid = (rng.random((B, H, W)) > 0.05).astype(np.uint8)
    src = rng.uniform(-300, 300, (B, C, H, W)).astype(f32) if C else None   # some beyond vmax = 255
    if family == "seam":
        flow[:, 0] += f32(W - 2.25)
        flow[:, 0, :, ::3] -= f32(2 * W)
    elif family == "pole":
        flow[:, 1, : H // 2] -= f32(3.0)
        flow[:, 1, H // 2:] += f32(3.0)
    elif family == "collapse":
        flow[:, 0] = (W // 2 + 0.5 - xs).astype(f32)
        flow[:, 1] = (H // 2 + 0.25 - ys).astype(f32)
    elif family == "two_layers":
        # even columns are the far layer (d = 1) and stay, odd columns the near layer (d = 4) and move one column left onto them
        flow[:] = 0
        flow[:, 0, :, 1::2] = -1
        d[:] = 1
        d[:, :, 1::2] = 4
        valid[:] = 1
        if C:
            src[:, :, :, 0::2] = -7.0
            src[:, :, :, 1::2] = (np.arange(C, dtype=f32)[None, :, None, None] + 10)
    elif family == "blend":
        flow[:] = 0
        flow[:, 0, :, 1::2] = -1
        d[:] = 1
        d[:, :, 1::2] = f32(1.125)                                        # inside 2^0.25: the two layers must blend
        valid[:] = 1
    elif family == "passthrough":
        flow[:] = 0
        valid[:] = 1
    elif family == "junk":
        bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -1.0], f32)
        pick = rng.integers(0, 12, (B, H, W))
        d = np.where(pick < 6, bad[np.minimum(pick, 5)], d).astype(f32)
        fl = rng.integers(0, 10, (B, 2, H, W))
        flow = np.where(fl < 5, bad[np.minimum(fl, 4)], flow).astype(f32)
        if C:
            sp = rng.integers(0, 10, (B, C, H, W))
            src = np.where(sp < 5, bad[np.minimum(sp, 4)], src).astype(f32)
        weight[:, ::5, ::3] = np.nan
        weight[:, 1::5, ::3] = -1
    else:
        raise ValueError(family)
    return src, flow, d, weight, valid


def junk_as_invalid(src, flow, d, weight, valid):
    """The same inputs with every pixel that holds a bad value declared invalid and its values replaced by harmless ones."""
    with np.errstate(invalid="ignore"):
        bad = ~((d >= 0) & (d < 2.0 ** 30)) | ~(weight > 0) | ~(np.abs(flow) < 2.0 ** 29).all(1)
        if src is not None:
            bad |= ~(np.abs(src) < 2.0 ** 30).all(1)
    clean = lambda a, m: np.where(m, np.float32(1), a).astype(np.float32)                                  # noqa: E731
    s2 = None if src is None else clean(src, bad[:, None])
    return s2, np.where(bad[:, None], np.float32(0), flow).astype(np.float32), clean(d, bad), clean(weight, bad), \
        np.where(bad, 0, valid).astype(np.uint8)


# ---- runners -------------------------------------------------------------------------------------------------------------------
def project_run(lib, inv_depth, weight, R, T, mask=None, device="cpu", n_min=1e-6):
    """pf_reproj_project on numpy inputs into buffers pre-filled with NaN / 255 -> (flow, d_new, valid) numpy."""
    B, H, W = inv_depth.shape
    flow = torch.full((B, 2, H, W), float("nan"), device=device)
    dn = torch.full((B, H, W), float("nan"), device=device)
    valid = torch.full((B, H, W), 255, dtype=torch.uint8, device=device)
    lib.reproj_project(_t(np.asarray(inv_depth, np.float32), device), _t(np.asarray(weight, np.float32), device), _t(mask, device),
                       _t(np.asarray(R, np.float32), device), _t(np.asarray(T, np.float32), device), flow, dn, valid, n_min)
    return flow.cpu().numpy(), dn.cpu().numpy(), valid.cpu().numpy()


class ZRun:
    """The three launches of a z-splat on buffers of its own, fed with numpy; every intermediate is kept."""

    def __init__(self, lib, B, C, H, W, device="cpu", offset=0):
        self.lib, self.device, self.shape = lib, device, (B, C, H, W)
        N = B * H * W
        # offset (in elements) shifts every map off its 16-byte alignment: the element form
        def buf(n, dtype, fill):
            return torch.full((n + offset,), fill, dtype=dtype, device=device)[offset:]
        self.acc = torch.zeros(B, C + 3, H, W, dtype=torch.int64, device=device)
        self.front = buf(N, torch.int32, 0).view(B, H, W)
        self.out = buf(N * C, torch.float32, float("nan")).view(B, C, H, W) if C else None
        self.d_out = buf(N, torch.float32, float("nan")).view(B, H, W)
        self.w_out = buf(N, torch.float32, float("nan")).view(B, H, W)
        self.hole = buf(N, torch.uint8, 255).view(B, H, W)

    def run(self, src, flow, d, weight, valid, **opt):
        """-> reproject_ref.zsplat's tuple."""
        o = dict(rr.DEFAULTS, **opt)
        dev, lib = self.device, self.lib
        t = [_t(x, dev) for x in (src, flow, d, weight, valid)]
        lib.zsplat_front(*t, self.front, o["b_min"])
        front = self.front.cpu().numpy().view(np.uint32).copy()
        lib.zsplat_accumulate(*t, self.front, self.acc, o["b_min"], o["ztol_log2"], o["w_max"], o["dmax"], o["vmax"])
        acc = self.acc.cpu().numpy().copy()
        lib.zsplat_resolve(self.acc, self.front, self.out, self.d_out, self.w_out, self.hole, o["cmin"], o["w_max"], o["dmax"], o["vmax"])
        n = lambda x: None if x is None else x.cpu().numpy().copy()                                     # noqa: E731
        return front, acc, n(self.out), n(self.d_out), n(self.w_out), n(self.hole), n(self.front).view(np.uint32), n(self.acc)


def zsplat_run(lib, src, flow, d, weight, valid, device="cpu", offset=0, **opt):
    B, H, W = d.shape
    return ZRun(lib, B, 0 if src is None else src.shape[1], H, W, device, offset).run(src, flow, d, weight, valid, **opt)


def same_bits(a, b, what):
    """Every element of two result tuples, bit for bit (None matches None)."""
    names = ("front", "sums", "out", "d_out", "w_out", "hole", "front after", "sums after")
    for name, x, y in zip(names, a, b):
        if x is None or y is None:
            assert x is None and y is None, (what, name)
            continue
        assert x.shape == y.shape and (bits(x) == bits(y)).all(), f"{what}: {name} differs in {int((bits(x) != bits(y)).sum())} elements"


def update_run(lib, d_s, w_s, d_m, w_m, disagree, flags, seg, device="cpu", offset=0, **opt):
    """pf_depth_update on copies -> (d, w, seg') numpy."""
    o = dict(rr.DEFAULTS, **opt)
    def shifted(a):
        a = np.ascontiguousarray(a)
        if not offset:
            return _t(a.copy(), device)
        return _t(np.concatenate([np.zeros(offset, a.dtype), a.reshape(-1)]), device)[offset:].view(a.shape)
    ds, ws, dm, wm = (shifted(np.asarray(x, np.float32)) for x in (d_s, w_s, d_m, w_m))
    dis = None if disagree is None else shifted(np.asarray(disagree, np.uint8))
    fl, sg = _t(np.asarray(flags, np.int32).copy(), device), _t(np.asarray(seg, np.int32).copy(), device)
    lib.depth_update(ds, ws, dm, wm, dis, fl, sg, o["tol_log2"], o["decay"], o["w_max"])
    return ds.cpu().numpy(), ws.cpu().numpy(), sg.cpu().numpy()


def update_inputs(B, H, W, seed=0):
    """State and measurement with every branch of the update: agreeing, far apart, one side missing, disagree set, junk."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    ds = np.exp2(rng.uniform(-3, 2, (B, H, W))).astype(f32)
    dm = (ds * np.exp2(rng.choice([0.0, 0.125, -0.25, 0.4375, 1.0, -2.0, 0.75], (B, H, W)))).astype(f32)
    ws = (rng.integers(0, 150, (B, H, W)) / 16).astype(f32)
    wm = (rng.integers(0, 150, (B, H, W)) / 16).astype(f32)
    dis = (rng.random((B, H, W)) < 0.1).astype(np.uint8)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1.0, 0.0], f32)
    for a in (ds, dm, ws, wm):
        k = rng.integers(0, 40, (B, H, W))
        a[k < 6] = bad[k[k < 6]]
    return ds, ws, dm, wm, dis


# ---- scenes and paths ------------------------------------------------------------------------------------------------------------
CONVEX = rr.Scene(4.0)
_C0 = np.array([0.25, -0.1, 0.05])
# a ball of radius 0.42 two units ahead of camera 0: the camera then steps sideways by 0.29 of the nearest depth (1.58), which moves
# the ball by more than its angular radius, so part of its new silhouette lies over what was background
OCCLUDER = rr.Scene(4.0, ball=(_C0 + np.array([2.0, 0.0, 0.0]), 0.42))
OCCLUDER_CAMERAS = ((np.eye(3), _C0), (er.axis_angle((1, 2, 3), 2.0), _C0 + np.array([0.0, 0.29 * 1.58, 0.02])))
OCCLUDER_SHAPES = TRUTH_SHAPES + ((64, 128),)
TAP_REACH = 0.75           # a used tap has b_k >= b_min = 0.25, so its sample lies within 3/4 px of the target on both axes
ZTOL = 2.0 ** 0.25


def occluder_pair(H, W):
    """(inv depth of frame 0, of frame 1, info, R, T) of the occluder scene.  info judges the WHOLE new silhouette of the ball:
      region   [H,W] bool: the pixels of frame 1 that show the ball;
      reached  [H,W] bool: a ball sample of frame 0 has a used tap there (from the float64 projection of the true depth; where none
               has, no forward splat can put the ball's depth, and the share of such pixels is capped instead);
      spread   [H,W]: how far the inverse depth of the samples that may be blended at the pixel can lie from the pixel's own.  What
               a target blends are samples within TAP_REACH px of it that the z-test admits, each carrying the exact inverse depth of
               the ball point it shows: the ball's near side over that footprint (the limb's value where the footprint leaves the
               ball), and its far side where frame 0 saw it and it lies within ZTOL of the footprint's smallest near value.  A mean
               of such values lies between their extremes, so |out - truth| <= spread + the convex scene's cap on top."""
    cam0, cam1 = OCCLUDER_CAMERAS
    rho0, on0, _ = OCCLUDER.depth(*cam0, H, W)
    rho1, on1, _ = OCCLUDER.depth(*cam1, H, W)
    R, T = rr.relative_pose(cam0, cam1)
    R32, T32 = R.astype(np.float32)[None], T.astype(np.float32)[None]
    d0 = 1.0 / rho0
    # where the ball samples of frame 0 land
    flow, _, _, _, _ = rr.project(d0.astype(np.float32)[None], np.ones((1, H, W), np.float32), R32, T32)
    m, n = er.grid(H, W)
    qx, qy = (m + flow[0, 0])[on0], (n + flow[0, 1])[on0]
    x0, y0 = np.floor(qx), np.floor(qy)
    fx, fy = qx - x0, qy - y0
    reached = np.zeros((H, W), bool)
    for dy, dx, bk in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)), (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
        yy, xx = (y0 + dy).astype(int), np.mod(x0 + dx, W).astype(int)
        use = (bk >= 0.25) & (yy >= 0) & (yy < H)
        reached[yy[use], xx[use]] = True
    # the extremes of what may be blended at each pixel of the silhouette
    to = OCCLUDER.ball[0] - cam1[1]
    limb = 1.0 / np.sqrt(to @ to - OCCLUDER.ball[1] ** 2)
    off = np.linspace(-TAP_REACH - 1e-3, TAP_REACH + 1e-3, 25)
    oy, ox = np.meshgrid(off, off, indexing="ij")
    spread = np.zeros((H, W))
    for y, x in zip(*np.nonzero(on1)):
        rho, on, far = OCCLUDER.depth(*cam1, H, W, at=(x + ox, y + oy))
        near = 1.0 / rho[on]
        vals = [near, [limb] if not on.all() else []]
        back = 1.0 / far[on]
        vals.append(back[back >= near.min() / ZTOL])
        vals = np.concatenate([np.asarray(v, np.float64).ravel() for v in vals])
        spread[y, x] = np.abs(vals - 1.0 / rho1[y, x]).max()
    info = dict(region=on1, reached=reached & on1, spread=spread, was_background=on1 & ~on0)
    return d0, 1.0 / rho1, info, R32, T32


def occluder_unjudged_cap(H, W):
    """The share of the silhouette that may go unjudged: HOLE_CAP of it as anywhere, and half of its rim.  A rim target has the
    ball on one side only, so half of the sub-pixel offsets that would reach it belong to samples of the background; a ring one
    pixel wide is 2 / a of a disc of radius a pixels (all of it for a <= 2)."""
    to = OCCLUDER.ball[0] - OCCLUDER_CAMERAS[1][1]
    a = np.arcsin(OCCLUDER.ball[1] / np.linalg.norm(to)) * W / (2 * np.pi)
    return HOLE_CAP + 0.5 * min(1.0, 2.0 / a)


def occluder_error(d_out, hole, truth, info, cap):
    """(worst |d_out - truth| / (cap truth + spread) over the judged pixels of the silhouette, the share of the silhouette that is
    not judged, the number of judged pixels).  Judged: a ball sample reaches the pixel and the output is no hole (a single tap
    below cmin leaves one)."""
    k = info["reached"] & (hole == 0)
    err = np.abs(d_out[k] - truth[k]) / (cap * truth[k] + info["spread"][k])
    return float(err.max()), 1.0 - k.sum() / info["region"].sum(), int(k.sum())


def camera(k):
    """Camera k of the six-frame path: 0.27 from the centre to begin with, steps of 0.2 to 0.3 along a gentle curve (the nearest
    wall stays beyond 2.5, so a baseline is below 0.3 of the minimum depth), turning
    2 degrees per frame about a tilted axis."""
    u = np.array([0.8, 0.5, 0.33]) / np.linalg.norm([0.8, 0.5, 0.33])
    c = np.array([0.25, -0.1, 0.05]) + 0.2 * k * u + 0.01 * k * k * np.array([-0.5, 0.8, 0.1])
    return er.axis_angle((1, 2, 3), 2.0 * k), c


def pair(scene, k, H, W):
    """(inv depth of frame k, inv depth of frame k + 1, on-ball mask of frame k + 1, R, T) float64 / fp32 pose of the step k -> k + 1."""
    c0, c1 = camera(k), camera(k + 1)
    rho0, _, _ = scene.depth(*c0, H, W)
    rho1, on1, _ = scene.depth(*c1, H, W)
    R, T = rr.relative_pose(c0, c1)
    return 1.0 / rho0, 1.0 / rho1, on1, R.astype(np.float32)[None], T.astype(np.float32)[None]


def rel_error(d_out, hole, truth, where=None):
    """(worst |d_out / truth - 1| over the pixels that are no hole (and in `where`), the share of holes)."""
    keep = hole == 0 if where is None else (hole == 0) & where
    return float(np.abs(d_out[keep] / truth[keep] - 1).max()), float((hole != 0).mean())


def filter_path(run_update, run_reproject, H, W, seed, sigma=FILTER_SIGMA, frames=6):
    """The recursive filter along the six-frame path through the convex scene, each measurement the true inverse depth times
    2^(sigma g), g standard normal: (rms log2 error of the filtered map at the last frame, that of the last measurement alone)."""
    rng = np.random.default_rng(seed)
    ds, ws = np.zeros((1, H, W), np.float32), np.zeros((1, H, W), np.float32)
    flags, seg = np.array([[0, 1, 1, 1]], np.int32), np.array([1], np.int32)
    for k in range(frames):
        d0, _, _, R, T = pair(CONVEX, k, H, W)
        meas = (d0 * np.exp2(sigma * rng.standard_normal((H, W)))).astype(np.float32)[None]
        ds, ws = run_update(ds, ws, meas, np.ones_like(meas), None, flags, seg)
        if k == frames - 1:
            ok = ws[0] > 0
            return float(np.sqrt(np.mean(np.log2(ds[0][ok] / d0[ok]) ** 2))), float(np.sqrt(np.mean(np.log2(meas[0] / d0) ** 2)))
        ds, ws = run_reproject(ds, ws, R, T)


def lib_filter(lib, device="cpu"):
    """filter_path's two steps through the entry points of `lib`."""
    def upd(ds, ws, dm, wm, dis, flags, seg):
        return update_run(lib, ds, ws, dm, wm, dis, flags, seg, device)[:2]

    def rep(ds, ws, R, T):
        flow, dn, valid = project_run(lib, ds, ws, R, T, None, device)
        r = zsplat_run(lib, None, flow, dn, ws, valid, device)
        return r[3], r[4]
    return upd, rep


def ref_filter(fault=None):
    def upd(ds, ws, dm, wm, dis, flags, seg):
        return rr.update(ds, ws, dm, wm, dis, flags, seg, np.float32, fault)[:2]

    def rep(ds, ws, R, T):
        r = rr.reproject(None, ds, ws, R, T, fault=fault)
        return r[3], r[4]
    return upd, rep
