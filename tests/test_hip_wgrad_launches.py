"""Every weight-gradient launch of a training step, checked against float64 (tests/wgrad_launches.py).

A real training forward + backward runs eagerly under a recorder of PfLib.conv2d_wgrad / PfLib.conv2d_wgrad_small -- once through
plain .backward() and once through the product's train_step with the gradient sink on (the stems accumulate straight into
.grad) --, at the training crop (384x512, iters = 12: deferred launches over 12 images of 48x64, many tiles per split) and at
136x216, iters = 4 (a 17x27 map, ragged on both axes).  Each distinct launch signature is then replayed on fresh seeded buffers
with the recorded layout, at its recorded geometry and at a ragged sibling (H - 1, W - 3, same tile count and splits); dw, db,
the padding pattern of dw / db and the sentinels around the read slices are checked after one launch and after a second one
into the same buffers (2x).  A weight-gradient launch the product starts to make is checked here without anyone writing a
test for it."""
import argparse
import time

import pytest
import torch

import wgrad_launches as wl

pytestmark = pytest.mark.gpu

# (H, W, iters), B = 1, BatchNorm frozen as in bench.py's training leg; each once per path of PATHS
RUNS = [(384, 512, 12), (136, 216, 4)]
PATHS = ("backward", "train_step+sink")


def _model(dev):
    from prior_flow_amd import det_state_dict
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=False, dropout=0.0))
    m.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
    m = m.to(dev).train()
    m.freeze_bn()
    return m


@pytest.fixture(scope="module")
def recorded(monkeypatch_module):
    from prior_flow_amd import synthetic_pair
    from prior_flow_amd import train as tr
    from prior_flow_amd.autograd import SINK
    dev = torch.device("cuda:0")
    monkeypatch_module.setenv("PRIORFLOW_GRAD_SINK", "1")
    rec = wl.Recorder()
    with rec:                                   # installed before any model exists
        for H, W, iters in RUNS:
            for path in PATHS:
                rec.path = f"{path} {H}x{W} iters={iters}"
                model = _model(dev)
                i1, i2 = (t.to(dev) for t in synthetic_pair(1, H, W))
                if path == "backward":
                    assert not SINK.active
                    pa, pb = model(i1, i2, iters=iters)
                    (pa[-1].abs().sum() + pb[-1].abs().sum()).backward()
                    del pa, pb
                else:
                    args = argparse.Namespace(lr=1e-4, wdecay=5e-5, epsilon=1e-8, num_steps=1000, clip=1.0)
                    opt, sched = tr.fetch_optimizer(args, model)
                    gen = torch.Generator().manual_seed(5)
                    gt = (torch.rand(1, 2, H, W, generator=gen) * 6 - 3).to(dev)
                    valid = torch.ones(1, H, W, device=dev)
                    _, m = tr.train_step(model, opt, sched, tr.uniform_loss(H, W), i1, i2, gt, valid, iters=iters, clip=args.clip)
                    assert float(m["grad_norm"]) > 0 and not SINK.active
                    del opt, sched
                torch.cuda.synchronize()
                del model
                torch.cuda.empty_cache()
    assert rec.launches, "no weight-gradient launch was recorded"
    return rec.launches


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


def _by_signature(launches):
    sigs = {}
    for ln in launches:
        sigs.setdefault(ln.sig, []).append(ln)
    return sigs


def test_recorded_launches_cover_what_this_file_exists_for(recorded):
    """It must fail if the product stops launching one of these (the replay below would then no longer check it)."""
    mf = [ln.args for ln in recorded if ln.kind == "mfma"]
    sm = [ln.args for ln in recorded if ln.kind == "small"]
    shapes = {(a["kh"], a["kw"]) for a in mf}
    assert {(3, 3), (1, 5), (5, 1), (1, 1)} <= shapes, shapes
    assert any(a["c1"] > 0 for a in mf), "no two-segment launch"
    assert any(a["off_dy"] > 0 and a["ld_dy"] > a["cout"] for a in mf), "no launch with off_dy > 0 inside a wider dy row"
    couts = sorted({a["cout"] for a in mf})
    assert any(c < 32 for c in couts) and any(c % 128 for c in couts), couts
    cins = sorted({a["c0"] + a["c1"] for a in mf})
    assert any(c < 32 for c in cins) and any(c % 32 for c in cins), cins
    assert any(a["nchw"] and a["stride"] == 2 and a["cin"] == 3 for a in sm), "no NCHW stride-2 cin-3 stem launch"
    offs = {a["off_in"] for a in sm if not a["nchw"] and a["stride"] == 1 and a["cin"] == 2}
    assert {0, 2} <= offs, f"channel-last stride-1 cin-2 stem launches at off_in {sorted(offs)}"
    # the regime the directed cases cannot guarantee for the product: splits that own several tiles, unevenly
    multi = [ln for ln in recorded if ln.kind == "mfma" and wl.tiles(ln) > wl.mfma_splits(ln)]
    assert any(wl.tiles(ln) % wl.mfma_splits(ln) for ln in multi), "no MFMA launch with unevenly shared pixel tiles"
    paths = {ln.path.split(" ")[0] for ln in recorded}
    assert paths == set(PATHS), paths


def test_every_recorded_wgrad_launch_matches_fp64(recorded):
    from prior_flow_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    sigs = _by_signature(recorded)
    checked, failures, rows = set(), [], []
    worst_kind = {}
    t_start = time.time()
    for idx, (sig, launches) in enumerate(sorted(sigs.items(), key=lambda kv: wl.sig_str(kv[1][0]))):
        ln = launches[0]
        geos = [("recorded", (ln.B, ln.H, ln.W))]
        sib = wl.ragged_sibling(ln)
        if sib:
            geos.append(("ragged", sib))
        worst = {"dw": (0.0, 0.0), "db": (0.0, 0.0)}
        t0 = time.time()
        for gname, (b, h, w) in geos:
            case = wl.build_case(ln, b, h, w, dev, seed=2000 + idx)
            ref = wl.reference(case)
            for mult in (1.0, 2.0):            # the second launch accumulates into the same buffers
                wl.run_case(lib, case)
                fails, wr = wl.check_case(case, ref, mult)
                worst = {k: tuple(max(a, b_) for a, b_ in zip(worst[k], wr[k])) for k in worst}
                failures += [f"[{wl.sig_str(ln)}] {gname} {b}x{h}x{w} x{mult:g}: {f}" for f in fails]
            del case, ref
        torch.cuda.empty_cache()
        checked.add(sig)
        wk = worst_kind.setdefault(ln.kind, {"dw": [0.0, 0.0], "db": [0.0, 0.0], "n": 0})
        wk["n"] += 1
        for k in ("dw", "db"):
            wk[k] = [max(a, b_) for a, b_ in zip(wk[k], worst[k])]
        split = f"tiles {wl.tiles(ln)}" + (f" splits {wl.mfma_splits(ln)}" if ln.kind == "mfma" else "")
        paths = sorted({l.path for l in launches})
        rows.append(f"{idx:3d} {wl.sig_str(ln)}  ({split})\n      geometries " + ", ".join(f"{gn} {b}x{h}x{w}" for gn, (b, h, w) in geos) +
                    ("" if sib else "; no ragged sibling: H - 1, W - 3 changes the tile count") +
                    f"\n      worst |err| / bound: dw per-element {worst['dw'][0]:.3g} aggregate {worst['dw'][1]:.3g}, "
                    f"db per-element {worst['db'][0]:.3g} aggregate {worst['db'][1]:.3g}"
                    f"  ({time.time() - t0:.1f} s; {len(launches)} launches in: {'; '.join(paths)})")
    print(f"\n{len(checked)} weight-gradient launch signatures checked against float64 in {time.time() - t_start:.0f} s:")
    print("\n".join(rows))
    for kind, wk in sorted(worst_kind.items()):
        print(f"worst of the {wk['n']} {kind} signatures: dw per-element {wk['dw'][0]:.3g} aggregate {wk['dw'][1]:.3g}, "
              f"db per-element {wk['db'][0]:.3g} aggregate {wk['db'][1]:.3g}")
    assert checked == set(sigs)
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:200])
