"""CPU checks of tests/train_loop_ref.py, the harness of test_hip_train_loop.py: the float64 reference pinned to a run's saved
state, the bounds the bf16 hi + lo rounding model gives, and proof that both have teeth -- before any GPU is involved.  The
"kernel" here is the plain float32 run of the same loop body; its own masks, coordinates and sampled values are the saved state.
No GPU."""
import pytest
import torch

import train_loop_ref as tl

CASES = {c.name: c for c in (tl.EVEN, tl.RAGGED, tl.EVEN_LAST, tl.EVEN_B)}
FAULT_CASE = tl.RAGGED
_CACHE = {}


def _case(name):
    """inputs, the float32 run (gradients, predictions, state) and the pinned (reference, model) of one case: computed once,
    shared by the tests below and never modified."""
    if name not in _CACHE:
        torch.manual_seed(0)
        case = CASES[name]
        inputs = tl.make_inputs(case)
        got, preds, state = tl.evaluate(case, inputs, "cpu", torch.float32, tl.conv_plain)
        ref, model, ref_preds = tl.reference_and_model(case, inputs, state, "cpu")
        _CACHE[name] = dict(case=case, inputs=inputs, got=got, preds=preds, state=state, ref=ref, model=model, ref_preds=ref_preds)
    return _CACHE[name]


def test_conv_taps_is_conv2d():
    """The per-tap convolution both precisions run == torch's conv2d, values and all three gradients (float64)."""
    g = torch.Generator().manual_seed(2)
    for kh, kw, ci in ((3, 3, 5), (1, 5, 4), (5, 1, 4), (1, 1, 6), (7, 7, 2)):
        pad = (kh // 2, kw // 2)
        args = [torch.randn(2, ci, 6, 7, generator=g, dtype=torch.float64), torch.randn(3, ci, kh, kw, generator=g, dtype=torch.float64),
                torch.randn(3, generator=g, dtype=torch.float64)]
        gy = torch.randn(2, 3, 6, 7, generator=g, dtype=torch.float64)
        res = []
        for fn in (lambda x, w, b: tl.conv_taps(x, w, b, pad), lambda x, w, b: torch.nn.functional.conv2d(x, w, b, padding=pad)):
            leaves = [a.clone().requires_grad_(True) for a in args]
            y = fn(*leaves)
            res.append([y.detach()] + list(torch.autograd.grad(y, leaves, gy)))
        for a, b in zip(*res):
            assert torch.allclose(a, b, rtol=1e-12, atol=1e-12), (kh, kw)


def test_split_model_rounds_all_three_passes():
    """_ConvSplit: forward, data gradient and weight gradient are those of operands rounded to bf16 hi + lo (16 significant
    bits: relative error <= 2^-16, and not fp32-exact); the 2-channel stems stay plain fp32."""
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(2, 8, 5, 6, generator=g), torch.randn(4, 8, 3, 3, generator=g), torch.randn(4, generator=g)
    gy = torch.randn(2, 4, 5, 6, generator=g)
    r = tl.split_round
    assert float(((r(x) - x).abs() / x.abs()).max()) <= 2.0 ** -16 and float((r(x) - x).abs().max()) > 0
    leaves = [t.clone().requires_grad_(True) for t in (x, w, b)]
    y = tl.conv_split(*leaves, (1, 1))
    dx, dw, db = torch.autograd.grad(y, leaves, gy)
    F = torch.nn.functional
    assert torch.allclose(y, F.conv2d(r(x), r(w), b, padding=1), rtol=0, atol=1e-5)
    assert torch.allclose(dx, torch.nn.grad.conv2d_input(x.shape, r(w), r(gy), padding=1), rtol=0, atol=1e-5)
    assert torch.allclose(dw, torch.nn.grad.conv2d_weight(r(x), w.shape, r(gy), padding=1), rtol=0, atol=1e-5)
    assert torch.allclose(db, gy.sum((0, 2, 3)), rtol=0, atol=1e-5)
    assert not torch.equal(y, tl.conv_plain(x, w, b, (1, 1)))
    x2, w2 = torch.randn(1, 2, 5, 6, generator=g), torch.randn(4, 2, 7, 7, generator=g)
    assert torch.equal(tl.conv_split(x2, w2, b, (3, 3)), tl.conv_plain(x2, w2, b, (3, 3)))


@pytest.mark.parametrize("name", [tl.EVEN.name, tl.RAGGED.name, tl.EVEN_LAST.name, tl.EVEN_B.name])
def test_float32_run_is_within_the_bounds_of_its_pinned_reference(name):
    """At the shapes and seeds of test_hip_train_loop.py every gradient of the plain float32 run is within its bound, the seam
    cap holds (the committed seeds are chosen so that it does) and the pinned reference reproduces the run's predictions."""
    c = _case(name)
    case = c["case"]
    assert len(c["state"]) == case.iters and set(c["state"][0]) == set(tl.VALUES + tl.RELUS_A + tl.RELUS_B)
    assert set(c["ref"]) == set(c["got"]) and len(c["ref"]) == 6 + 8 + 2 * (19 + 15)
    fails, report = tl.check(c["got"], c["ref"], c["model"])
    e_t = sorted(v[2] for v in report.values())
    print(f"{name}: float32 run, worst err / bound: {tl.worst(report)}; E_t median {e_t[len(e_t) // 2]:.1e} worst {e_t[-1]:.1e}")
    assert not fails, fails
    # several pixels of initial flow: lookups do cross the seam (x outside [0, W8 - 1] for some window samples)
    x = c["state"][0]["c_a"][:, 0]
    assert float(x.min()) < 0 and float(x.max()) > case.W8 - 1
    for a, b in zip(c["preds"], c["ref_preds"]):
        assert tl.mean_epe(a, b) < 1e-3
    if case.last_only:
        assert all(float(s.abs().max()) == 0 for k, s in enumerate(c["inputs"]["seeds"]) if k not in (case.iters - 1, 2 * case.iters - 1))


def test_bounds_are_rounding_sized():
    """E_t, the rounding model's distance from the reference, is what 16-bit operands give (median above 1e-6, worst below
    1e-4), and the BOUND of every tensor with a non-zero gradient is below 1e-3 of its own norm -- the small ones (d_f1 / d_f2
    of norm 0.03 beside weight gradients of norm 5.8e3, the pyramid levels, conv_conf1) included: nothing of another tensor's
    size enters it.  Two orders below what the end-to-end tests allow."""
    for name in (tl.EVEN.name, tl.RAGGED.name, tl.EVEN_LAST.name):
        c = _case(name)
        _, report = tl.check(c["got"], c["ref"], c["model"])
        live = {k: v for k, v in report.items() if float(c["ref"][k].abs().max()) > 0}
        assert len(live) == len(report)             # no output of this harness has a true gradient of zero
        e_t = sorted(v[2] for v in live.values())
        assert 1e-6 < e_t[len(e_t) // 2] and e_t[-1] < 1e-4, (e_t[0], e_t[len(e_t) // 2], e_t[-1])
        rel = {k: v[3] for k, v in live.items()}
        print(f"{name}: bound / |ref| worst {max(rel.values()):.1e} ({max(rel, key=rel.get)}), d_f1a {rel['d_f1a']:.1e}, "
              f"pyr_a0 {rel['pyr_a0']:.1e}")
        assert max(rel.values()) < 1e-3, sorted(rel.items(), key=lambda kv: -kv[1])[:3]


# fault -> the output that must catch it (the table of measured ratios is in the test's docstring)
FAULT_TABLE = {
    "flaw_ba_detached": "d_f2a",
    "warp2_reads_conf_0_4": "d_f2a",
    "mask_quarter_missing": "d_net_a",
    "b_out_124_125_zero": "update_block.encoder.conv.weight",
    "d_inp_last_only": "d_inp_a",
    "cross_detached": "pyr_b0",
    "hidden_not_handed_on": "d_net_a",
    "stale_relu_mask": "ODDC.encoder.convc1_A.weight",
    "d_c1_tile_zero": "ODDC.encoder.convc1_A.weight",
}


@pytest.mark.parametrize("fault", tl.FAULTS)
def test_seeded_fault_is_caught_ten_times_over(fault):
    """Nine wrong backwards, each seeded into the float32 run with tensor hooks / detach (none changes a forward value, so the
    saved state and the reference are those of the clean run): the named output lands at least 10x beyond its bound.

    Measured on the CPU at B=1, 17x27, 4 iterations.  "old metric" is what the end-to-end tests assert to 2e-2 / 3e-2: the worst
    diff / (norm + 1e-3 * total) over the parameter gradients -- here the update blocks' only; a fault that touches nothing but
    leaf or pyramid gradients leaves it at the clean run's 4.6e-07, and in the full model reaches fnet through d_f1 / d_f2 of
    norm 0.02 beside the pyramids' 0.5.

      fault                                                     caught by                          err / bound   old metric
      --------------------------------------------------------  ---------------------------------  -----------   ----------
      (none)                                                    worst: flow_head.conv2.bias               0.18      4.6e-07
      flaw_ba detached (second pf_warp_gcorr_bwd missing)       d_f2a                                   11 655      4.6e-07
      second warp's gradient from conf columns 0:4              d_f2a (d_f1a alike)                     16 251      4.6e-07
      mask head's 0.25 missing in the data gradient (A)         d_net_a (ODDC.mask.0.bias: 109 041)     26 839      2.9e+00
      branch B's d_out columns 124, 125 zeroed                  update_block.encoder.conv.weight         3 680      1.5e-01
      d_inp from the last iteration only                        d_inp_a                                 18 980      4.6e-07
      A's cross lookup detached (nothing to B's pyramid)        pyr_b0 (pyr_b3: 12 323)                  8 464      4.6e-07
      hidden-state gradient not handed from iteration 1 to 0    d_net_a                                  6 462      1.9e-01
      convc1_A's ReLU mask of iteration 1 taken from 0 (stale)  ODDC.encoder.convc1_A.weight             1 789      5.0e-02
      rows 4:8 x columns 8:24 of d_c1 of iteration 1 zeroed     ODDC.encoder.convc1_A.weight             2 652      7.4e-02

    The last one is a tile strictly inside the 17x27 map (a 4x32 tile of the kernels would span its whole width).
    """
    c = _case(FAULT_CASE.name)
    got, preds, state = tl.evaluate(c["case"], c["inputs"], "cpu", torch.float32, tl.conv_plain, fault=fault)
    for a, b in zip(preds, c["preds"]):
        assert torch.equal(a, b)
    fails, report = tl.check(got, c["ref"], c["model"])
    key = FAULT_TABLE[fault]
    top = max(report.items(), key=lambda kv: kv[1][0])
    print(f"{fault}: {key} err / bound {report[key][0]:.1f} (worst: {top[0]} {top[1][0]:.1f}); old metric {tl.old_metric(got, c['ref']):.1e}")
    assert report[key][0] >= 10.0, (fault, key, report[key])
    assert fails


def test_without_the_pins_two_correct_runs_differ_beyond_the_bounds():
    """The float64 loop run FREE (its own ReLU masks, coordinates and sampled values) against the same float32 run: ReLU masks
    flip, derived sample coordinates cross the seam, and gradients differ far beyond rounding.  The pins are what make a
    rounding-sized bound possible; they are not redundant."""
    c = _case(tl.RAGGED.name)
    free, _, _ = tl.evaluate(c["case"], c["inputs"], "cpu", torch.float64, tl.conv_plain)
    fails, report = tl.check(c["got"], free, c["model"], model_ref=c["ref"])
    print(f"unpinned float64 reference: worst err / bound: {tl.worst(report)}")
    assert fails and max(v[0] for v in report.values()) > 1.0
