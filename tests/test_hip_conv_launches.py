"""Every pf_conv2d launch the product makes, checked against float64 (tests/conv_launches.py).

The product paths below run eagerly under a recorder of PfLib.conv2d; each distinct launch signature (precision, kernel shape,
planned tile / roles, groups, operand and output forms, epilogue and options) is then replayed on fresh seeded buffers with the
recorded layout -- at its product geometry and at a ragged sibling geometry the planner maps to the same signature -- and every
output form, the fused statistics and the sentinels around the written columns are checked.  A new kernel path the product
starts to launch is checked here without anyone writing a test for it.

The kernel a launch runs is the planner's choice from work-item counts, so the same layout runs other code at another image
size or batch.  test_every_reachable_plan_matches_fp64 therefore asks the host planners which (tile, roles) every recorded
layout reaches over the image sizes and batches the product supports (conv_launches.GRID) and replays each plan that no
recorded path produced, under the same bounds."""
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
             ("infer fp32", 1, 512, 1024, False, 0),
             # small maps: the layouts the engine builds only there, which the host sweep over geometries cannot invent
             ("infer bf16x3", 1, 128, 256, False, None), ("infer bf16x3", 2, 128, 256, False, None),
             ("infer mixed", 1, 128, 256, True, None), ("infer mixed", 2, 136, 216, True, None),
             ("infer fp32", 2, 136, 216, False, 0)]
TRAIN = ("train fwd+bwd", 1, 384, 512)
# a case bigger than this (output pixels x groups) is reduced to fewer images when the planner keeps its signature
MAX_PIXELS = 1 << 21
WALL = {}                                       # test name -> seconds, of this session (the two tables print both)


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
            rec.path, rec.image = f"{path} B{B} {H}x{W}", (B, H, W)
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
        rec.path, rec.image = f"{path} B{B} {H}x{W}", (B, H, W)
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
    WALL["recorded"] = time.time() - t_start
    print(f"\n{len(checked)} pf_conv2d launch signatures checked against float64 in {WALL['recorded']:.0f} s:")
    print("\n".join(rows))
    assert checked == set(sigs)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:200])


def _layout_of(sig):
    """A signature without the planner's choice (tile, roles): what reachable() holds fixed."""
    return sig[:3] + sig[5:]


def _is_encoder_layer1(ln):
    g = ln.groups[0]
    return (len(ln.groups) == 1 and g["kh"] == 3 and g["kw"] == 3 and g["c0"] == 64 and g["c1"] == 0 and g["cout"] == 64
            and (g["has_in_scale"] or g["has_stats_out"]))


def _is_small_f16(sig):
    return sig[0] == "f16" and sig[3:5] == ("tile3", "roles17")


def test_every_reachable_plan_matches_fp64(recorded):
    """Every (tile, roles) plan a recorded layout reaches on conv_launches.GRID and no recorded path produced, replayed once
    at its witness geometry under the bounds of test_every_recorded_launch_matches_fp64.

    The f16 plan of small maps (tile 3 / roles 17, pf_conv_dma_launch<1,2>) is one this test must see.  The recorded runs
    launch it themselves with every f16 layout the engine has (measured: sixteen signatures, ten of them at 1 x 512 x 1024, six
    more in the small-map runs of INFERENCE), so no such signature is left among the unrecorded ones.  Those the sweep reaches from a layout whose first recorded launch
    is on ANOTHER plan (measured: seven, from the 512 x 1024 runs' tile 4 / roles 18) are therefore replayed here as well,
    with that launch's own layout at the sweep's witness, and the test asserts that there is at least one: the sweep still
    has to find the plan by itself."""
    from prior_flow_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    t_start = time.time()                       # the host sweep counts
    have = set(_by_signature(recorded))
    plans_of = {}
    for s in have:
        plans_of.setdefault(_layout_of(s), set()).add((s[3], s[4]))
    # one sweep per distinct (descriptor layout, images per pair, resolution divisor)
    distinct = {}
    for ln in recorded:
        key = (_layout_of(ln.sig), cl.relation(ln), tuple(tuple(sorted(g.items())) for g in ln.groups))
        distinct.setdefault(key, ln)
    U = {}                                      # signature to replay (unrecorded, or of small_f16) -> (rank, launch, witness)
    small_f16 = set()                           # f16 tile 3 / roles 17 the sweep reaches from a launch recorded on another plan
    for ln in distinct.values():
        for sig, geos in cl.reachable(lib, ln).items():
            if sig in have and _is_small_f16(sig) and sig != ln.sig:
                small_f16.add(sig)              # recorded by another run of INFERENCE: replayed here all the same (docstring)
            elif sig in have:
                continue
            b, h, w, _ = cl.witness(lib, ln, sig, geos, ragged=False)
            # the same signature from several layers (the signature does not hold the channel counts): encoder layer 1 first
            # (asserted below), then the smallest replay
            rank = (0 if _is_encoder_layer1(ln) else 1, b * h * w * len(ln.groups))
            if sig not in U or rank < U[sig][0]:
                U[sig] = (rank, ln, geos)
    U = {sig: (rank, ln, cl.witness(lib, ln, sig, geos)) for sig, (rank, ln, geos) in U.items()}
    assert set(U) - have, "the sweep found no plan beyond the recorded ones: has the grid or the planner lost its thresholds?"
    checked, failures, rows, per_plan = set(), [], [], {}
    for idx, (sig, (_, ln, (B, H, W, ragged))) in enumerate(sorted(U.items(), key=lambda kv: cl.sig_str(kv[0]))):
        probe = cl.with_signature(ln, sig, B, H, W)
        ng = len(ln.groups)
        reduced = False
        while B > 1 and B * H * W * ng > MAX_PIXELS and cl.same_signature(lib, probe, B // 2, H, W):
            B //= 2
            reduced = True
        if B * H * W * ng > MAX_PIXELS:
            failures.append(f"[{cl.sig_str(sig)}] witness {B}x{H}x{W} x {ng} groups is above MAX_PIXELS = {MAX_PIXELS}")
            continue
        t0 = time.time()
        case = cl.build_case(lib, probe, B, H, W, dev, seed=5000 + idx)
        cl.run_case(lib, case)
        refs = cl.reference(case)
        fails, worst = cl.check_case(case, refs)
        failures += [f"[{cl.sig_str(sig)}] witness {B}x{H}x{W}: {f}" for f in fails]
        del case, refs
        torch.cuda.empty_cache()
        checked.add(sig)
        pw = per_plan.setdefault((sig[0], sig[3], sig[4]), {"elem": 0.0, "agg": 0.0, "n": 0})
        pw.update(elem=max(pw["elem"], worst["elem"]), agg=max(pw["agg"], worst["agg"]), n=pw["n"] + 1)
        g0 = ln.groups[0]
        rows.append(f"{idx:3d} {cl.sig_str(sig)}" + ("  (a recorded signature too)" if sig in have else "") + f"\n      layout {g0['c0'] + g0['c1']} -> {g0['cout']}, {cl.relation(ln)[0]} images per pair at 1/{cl.relation(ln)[1]}"
                    f" (from {ln.path}); recorded plans " + ", ".join(f"{t} {r}" for t, r in sorted(plans_of[_layout_of(sig)])) +
                    f"\n      witness {B}x{H}x{W}" + (" (ragged)" if ragged else " (not made ragged: no ragged geometry keeps the plan)") +
                    (" (B reduced, same signature)" if reduced else "") +
                    f"\n      worst |err| / bound: per-element {worst['elem']:.3g}, aggregate {worst['agg']:.3g}  ({time.time() - t0:.1f} s)")
    WALL["reachable"] = time.time() - t_start
    print(f"\n{len(checked) - len(small_f16)} pf_conv2d launch signatures beyond the {len(have)} recorded ones, and {len(small_f16)} recorded "
          f"f16 tile3 roles17 signatures reached from launches on another plan, from {len(distinct)} layouts over "
          f"{len(cl.GRID)} image geometries, checked against float64 in {WALL['reachable']:.0f} s"
          f" (the recorded signatures: " + (f"{WALL['recorded']:.0f} s" if "recorded" in WALL else "not run in this session") + "):")
    print("\n".join(rows))
    for (prec, tile, roles), pw in sorted(per_plan.items()):
        print(f"  worst of {prec} {tile} {roles} ({pw['n']} signatures): per-element {pw['elem']:.3g}, aggregate {pw['agg']:.3g}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:200])
    assert checked == set(U)
    # the two plans this test was written for (asserted after the replays, so that the table above is printed either way)
    assert any(_is_small_f16(s) for s in U), \
        "the sweep reaches no f16 launch on tile 3 / roles 17 from a launch recorded on another plan"
    assert any(s[3] == "tile5" and _is_encoder_layer1(U[s][1]) for s in U), \
        "no encoder layer 1 launch (3x3 64 -> 64 with in_scale or stats) on tile 5 among the unrecorded plans"
