"""Every pf_conv2d launch the product makes, checked against float64 (tests/conv_launches.py).

The product paths below run eagerly under a recorder of PfLib.conv2d; each distinct launch signature (precision, kernel shape,
planned tile / roles, groups, operand and output forms, epilogue and options) is then replayed on fresh seeded buffers with the
recorded layout -- at its product geometry and at a ragged sibling geometry the planner maps to the same signature -- and every
output form, the fused statistics and the sentinels around the written columns are checked.  A new kernel path the product
starts to launch is checked here without anyone writing a test for it."""
import argparse
import time

import pytest
import torch

import conv_launches as cl

pytestmark = pytest.mark.gpu

# (path, B, H, W, mixed_precision, model.precision): inference eagerly (use_graph False), iters=2
INFERENCE = [("infer bf16x3", 1, 512, 1024, False, None), ("infer bf16x3", 32, 512, 1024, False, None),
             ("infer bf16x3", 1, 640, 1280, False, None), ("infer bf16x3", 1, 136, 216, False, None),
             ("infer mixed", 1, 512, 1024, True, None), ("infer mixed", 32, 512, 1024, True, None),
             ("infer fp32", 1, 512, 1024, False, 0)]
TRAIN = ("train fwd+bwd", 1, 384, 512)
# a case bigger than this (output pixels x groups) is reduced to fewer images when the planner keeps its signature
MAX_PIXELS = 1 << 21


def _model(mixed, dev):
    from prior_flow_amd import det_state_dict
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=mixed, dropout=0.0))
    m.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
    return m.to(dev)


@pytest.fixture(scope="module")
def recorded():
    from prior_flow_amd import synthetic_pair
    dev = torch.device("cuda:0")
    rec = cl.Recorder()
    with rec:                                   # installed before any model or engine exists
        for path, B, H, W, mixed, prec in INFERENCE:
            rec.path = f"{path} B{B} {H}x{W}"
            model = _model(mixed, dev).eval()
            model.use_graph = False
            if prec is not None:
                model.precision = prec
            i1, i2 = synthetic_pair(B, H, W)
            with torch.no_grad():
                flow = model(i1.to(dev), i2.to(dev), iters=2, test_mode=True)
            torch.cuda.synchronize()
            assert torch.isfinite(flow).all()
            del model, flow
            torch.cuda.empty_cache()
        path, B, H, W = TRAIN
        rec.path = f"{path} B{B} {H}x{W}"
        model = _model(False, dev).train()
        model.freeze_bn()                       # as bench.py's training leg
        i1, i2 = synthetic_pair(B, H, W)
        pa, pb = model(i1.to(dev), i2.to(dev), iters=2)
        (pa[-1].abs().sum() + pb[-1].abs().sum()).backward()
        torch.cuda.synchronize()
        del model, pa, pb
        torch.cuda.empty_cache()
    assert rec.launches, "no pf_conv2d launch was recorded"
    return rec.launches


def _by_signature(launches):
    sigs = {}
    for ln in launches:
        sigs.setdefault(ln.sig, []).append(ln)
    return sigs


def test_recorded_paths_cover_the_kernel_matrix(recorded):
    """What the product launches must include the kernels this file exists for (a path that stops launching one of them
    would leave it untested here)."""
    sigs = set(_by_signature(recorded))
    tiles = {s[3] for s in sigs}
    roles = {s[4] for s in sigs}
    precs = {s[0] for s in sigs}
    epis = {g[0] for s in sigs for g in s[7]}
    opts = {o for s in sigs for g in s[7] for o in g[5]}
    assert {"tile3", "tile4", "tile5", "tile6", "tile7", "tile8"} <= tiles, tiles
    assert {"roles17", "roles18"} <= roles, roles
    assert {"fp32", "f16", "bf16x3"} <= precs, precs
    assert {"MASK", "ADD", "TANH_RELU", "GRU_ZR", "GRU_Q"} <= epis, epis
    assert {"save_gates", "out=h", "pre", "scale!=1"} <= opts, opts


def test_every_recorded_launch_matches_fp64(recorded):
    from prior_flow_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    sigs = _by_signature(recorded)
    checked, failures, rows = set(), [], []
    t_start = time.time()
    for idx, (sig, launches) in enumerate(sorted(sigs.items(), key=lambda kv: cl.sig_str(kv[0]))):
        ln = min(launches, key=lambda l: l.B * l.H * l.W)
        geos = [("product", (ln.B, ln.H, ln.W))]
        ng = len(ln.groups)
        B = ln.B
        while B > 1 and B * ln.H * ln.W * ng > MAX_PIXELS and cl.same_signature(lib, ln, B // 2, ln.H, ln.W):
            B //= 2
        if B != ln.B:
            geos[0] = ("product (B reduced, same signature)", (B, ln.H, ln.W))
        sib = cl.ragged_sibling(lib, ln)
        note = "" if sib else "no ragged sibling: " + cl.why_no_sibling(lib, ln)
        if sib:
            geos.append(("ragged", sib))
        worst = {"elem": 0.0, "agg": 0.0}
        t0 = time.time()
        for gname, (b, h, w) in geos:
            case = cl.build_case(lib, ln, b, h, w, dev, seed=1000 + idx)
            cl.run_case(lib, case)
            refs = cl.reference(case)
            fails, wr = cl.check_case(case, refs)
            worst = {k: max(worst[k], wr[k]) for k in worst}
            failures += [f"[{cl.sig_str(sig)}] {gname} {b}x{h}x{w}: {f}" for f in fails]
            del case, refs
        torch.cuda.empty_cache()
        checked.add(sig)
        paths = sorted({l.path for l in launches})
        rows.append(f"{idx:3d} {cl.sig_str(sig)}\n      geometries " +
                    ", ".join(f"{gn} {b}x{h}x{w}" for gn, (b, h, w) in geos) + (f"; {note}" if note else "") +
                    f"\n      worst |err| / bound: per-element {worst['elem']:.3g}, aggregate {worst['agg']:.3g}"
                    f"  ({time.time() - t0:.1f} s; {len(launches)} launches in: {'; '.join(paths)})")
    print(f"\n{len(checked)} pf_conv2d launch signatures checked against float64 in {time.time() - t_start:.0f} s:")
    print("\n".join(rows))
    assert checked == set(sigs)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:200])
