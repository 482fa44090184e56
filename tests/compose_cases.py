"""The cases of the chained-flow tests, run through any library handle (the host emulation on the CPU, the product's library on
the device): tests/test_compose_host.py and tests/test_hip_compose.py share them, tests/compose_ref.py judges them."""
import numpy as np
import torch

import compose_ref as cr

DENSE = [(kind, shape, wind) for kind in cr.KINDS for shape in cr.SHAPES for wind in cr.WINDS]


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")


def run_dense(lib, jobs, device=None, in_place=False):
    """pf_flow_compose on numpy jobs (f, state_f, g, occ_g) of one shape, one launch -> [(out, state_out)] numpy.  The outputs
    start poisoned (NaN, 0xFF); in_place: out = f and state_out = state_f."""
    ts = []
    for f, state_f, g, occ_g in jobs:
        f, state_f, g, occ_g = (_t(a, device) for a in (f, state_f, g, occ_g))
        if in_place:
            f = f.clone()                                # (on the CPU the tensor shares the caller's array)
            state_f = None if state_f is None else state_f.clone()
            if state_f is None:
                state_f = torch.zeros(f.shape[0], *f.shape[2:], dtype=torch.uint8, device=f.device)
            out, state_out = f, state_f
        else:
            out = torch.full_like(f, float("nan"))
            state_out = torch.full((f.shape[0],) + tuple(f.shape[2:]), 255, dtype=torch.uint8, device=f.device)
        ts.append((f, state_f, g, occ_g, out, state_out))
    lib.flow_compose(ts)
    return [(t[4].cpu().numpy(), t[5].cpu().numpy()) for t in ts]


def run_points(lib, pos, state, flow, occ, device=None):
    """pf_track_points on numpy pos [B,N,2], state [B,N], flow [B,2,H,W], occ [B,H,W] or None -> (pos', state') numpy."""
    p, s, f, o = (_t(a, device) for a in (pos.copy(), state.copy(), flow, occ))
    lib.track_points(p, s, f, o)
    return p.cpu().numpy(), s.cpu().numpy()


def check_dense_case(lib, kind, shape, wind, device=None):
    """One case of DENSE against the float64 restatement; returns the figures per image."""
    B, H, W = shape
    f, g, state, occ = cr.inputs(kind, B, H, W, wind)
    (out, st), = run_dense(lib, [(f, state, g, occ)], device)
    return [cr.check(out[b], st[b], cr.reference_dense(f[b], g[b], state[b], occ[b]), state[b], f"{kind} {shape} wind {wind} image {b}")
            for b in range(B)]


def sparse_points(B, H, W, N, seed=5):
    """pos [B,N,2] float32 and state [B,N]: the first points sit on the edges the statement names -- x in [W-1, W), x below 0,
    x above 2W, y below -0.5, y above H - 0.5 --, the rest are spread over and around the map; a few carry earlier bits."""
    g = np.random.default_rng(seed + N)
    pos = np.stack([g.uniform(-1.5 * W, 3.5 * W, (B, N)), g.uniform(-2.0, H + 1.0, (B, N))], -1)
    edge = np.array([[W - 0.25, H / 2], [-0.75 * W - 0.3, 3.2], [2 * W + 5.6, H - 2.3], [W / 3 + 0.1, -1.7], [W / 2 + 0.4, H + 0.2]])
    pos[:, :min(N, len(edge))] = edge[:min(N, len(edge))]
    state = np.where(g.random((B, N)) < 0.2, g.integers(1, 16, (B, N)), 0).astype(np.uint8)
    return pos.astype(np.float32), state


def check_sparse_case(lib, kind, shape, N, device=None):
    B, H, W = shape
    _, g, _, occ = cr.inputs(kind, B, H, W, 0.0)
    pos, state = sparse_points(B, H, W, N)
    p, s = run_points(lib, pos, state, g, occ, device)
    return [cr.check(p[b].T, s[b], cr.reference_points(pos[b], g[b], state[b], occ[b]), state[b], f"sparse {kind} {shape} N {N} image {b}")
            for b in range(B)]


def grid_np(B, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    return np.broadcast_to(np.stack([x.ravel(), y.ravel()], -1), (B, H * W, 2)).copy()
