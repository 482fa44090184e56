"""The 360-degree training augmentation on the device: pf_augment_360 / pf_augment_convert and
prior_flow_amd.augment against PIL's stored single operations, the reference's stored FlowAugmentor_360 runs
(tests/golden/augment_360.npz) and the numpy restatement (tests/augment_ref.py); then the plumbing: batches, repeats, out=,
graph capture, guard bands, unaligned bases, the side-stream feeder.

Bars: brightness / contrast / saturation and HSV -> RGB alone bit for bit; anything containing RGB -> HSV under the cap (at most
0.5 % of bytes differ, a lone hue step by at most 7 levels, a chain by at most 28); flow and valid bit for bit.  Device and host
emulation are each held to the cap, not to each other; whether they are equal on every byte is printed.
"""
import shutil

import numpy as np
import pytest
import torch

import augment_cases as ac
import augment_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_hip()
    from prior_flow_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def emu():
    if shutil.which("g++") is None:
        return None
    import __graft_entry__ as ge
    from prior_flow_amd import _lib
    return _lib.PfLib(ge.build_emu_augment(), require_cuda=False,
                      optional=tuple(n for n in _lib.EXPORTS if not n.startswith("pf_augment")))


@pytest.fixture(scope="module")
def gold():
    return ac.golden()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _colour(lib, img, params):
    got = ac.run(lib, img[None], img[None], np.zeros(img.shape[:2] + (2,), np.float32)[None], params, DEV)
    assert np.array_equal(got[0], got[1])
    return got[0][0].transpose(1, 2, 0)


def _mixed_batch(gold, size, B):
    """B samples of one size with different modes: the stored cases of that size, then sampled rows."""
    from prior_flow_amd import augment as ag
    H, W = size
    cases = [c for c in ac.CASES if c[1] == size]
    p = ag.AugmentParams(B)
    i1, i2, fl = [], [], []
    for b in range(B):
        c = cases[b % len(cases)]
        img, flow = ac.case_inputs(gold, c)
        ac.case_params(c, out=p, b=b)
        i1.append(np.roll(img[0], b, axis=0)); i2.append(np.roll(img[1], b, axis=0)); fl.append(np.roll(flow, b, axis=0))
    return np.stack(i1), np.stack(i2), np.stack(fl), p


# ---- bars 1 and 2: single operations -------------------------------------------------------------------------------------------
def test_single_operations_are_pil_bit_for_bit(lib, gold):
    for k, img in enumerate(gold["op_in"]):
        for op in range(3):
            for j, f in enumerate(ac.OP_FACTORS):
                assert np.array_equal(_colour(lib, img, ac.one_op_params(op, f)), gold["op_out"][k, op, j]), (op, k, f)


def test_hsv_conversions(lib, gold):
    out = torch.zeros(gold["hsv_in"].shape, dtype=torch.uint8, device=DEV)
    lib.augment_convert(_t(gold["hsv_back_in"]), out, True)
    assert np.array_equal(out.cpu().numpy(), gold["hsv_back_out"])                    # HSV -> RGB: bit for bit
    lib.augment_convert(_t(gold["hsv_in"]), out, False)
    share, worst = ac.image_diff(out.cpu().numpy()[..., 0], gold["hsv_out"][..., 0])
    print(f"RGB -> HSV on the device: hue plane differs on {share:.2e} of the pixels, by at most {worst:.0f}")
    assert share <= ac.CAP_SHARE and worst <= 1
    assert np.array_equal(out.cpu().numpy()[..., 1:], gold["hsv_out"][..., 1:])       # saturation and value


def test_hue_step_alone(lib, emu, gold):
    for k, img in enumerate(gold["op_in"]):
        for j, s in enumerate(ac.HUE_SHIFTS):
            p = ac.one_op_params(3, shift=s)
            got = _colour(lib, img, p)
            share, worst = ac.image_diff(got, gold["hue_out"][k, j])
            same = None if emu is None else np.array_equal(got, ac.run(emu, img[None], img[None], np.zeros((1,) + img.shape[:2] + (2,), np.float32), p)[0][0].transpose(1, 2, 0))
            print(f"hue step alone, image {k}, shift {s}: share {share:.2e}, worst {worst:.0f}; equal to the emulation: {same}")
            assert share <= ac.CAP_SHARE and worst <= ac.CAP_HUE


# ---- bars 2, 3, 4, 5: the stored reference runs through the sampler ----------------------------------------------------------
@pytest.mark.parametrize("case", ac.CASES, ids=[c[0] for c in ac.CASES])
def test_stored_reference_runs(lib, emu, gold, case):
    name, (H, W), seed, asym_roll, identity, _ = case
    img, flow = ac.case_inputs(gold, case)
    p = ac.case_params(case)
    row = p.row(0)
    w1, w2, wf, wv = ac.case_expected(gold, case)
    g1, g2, gf, gv = (o[0] for o in ac.run(lib, img[:1], img[1:], flow[None], p, DEV))
    share, worst = ac.image_diff(np.stack([g1, g2]), np.stack([w1, w2]))
    same = None
    if emu is not None:
        e = [o[0] for o in ac.run(emu, img[:1], img[1:], flow[None], p)]
        same = all(np.array_equal(a, b, equal_nan=True) for a, b in zip((g1, g2, gf, gv), e))
    print(f"case {name}: share of differing bytes {share:.2e}, worst {worst:.0f}; equal to the emulation on every byte: {same}")
    assert share <= ac.CAP_SHARE and worst <= ac.CAP_CHAIN
    if identity:
        assert share == 0.0                                  # no RGB -> HSV in the chain: bit for bit
        inside = np.zeros((H, W), bool)
        for x0, y0, dx, dy in row["rects"]:
            inside[y0:y0 + dy, x0:x0 + dx] = True
        inside = np.roll(inside, row["r2"], axis=1)
        assert np.array_equal(g1, np.roll(img[0], row["r1"], axis=1).transpose(2, 0, 1))
        assert np.array_equal(g2[:, ~inside], np.roll(img[1], row["r2"], axis=1).transpose(2, 0, 1)[:, ~inside])
    with np.errstate(invalid="ignore"):
        ref = ar.augment_sample(img[0], img[1], flow, row)
    wf, wv = (ref[2], ref[3]) if wf is None else (wf, wv)    # identity cases: the restatement (their flows are not stored)
    assert ac.same_flow(gf, wf) and np.array_equal(gv, wv)
    assert (gv == 0).any() and (gv[np.isnan(gf).any(axis=0)] == 0).all()


@pytest.mark.parametrize("size", ac.SIZES, ids=ac.tag)
def test_hand_made_geometry(lib, gold, size):
    H, W = size
    img, flow = gold["smooth_" + ac.tag(size)], gold["flow_" + ac.tag(size)]
    mean = (img[1].reshape(-1, 3).astype(np.int64).sum(axis=0) // (H * W)).astype(np.float32)
    for what, rects, r1, r2 in ac.hand_cases(H, W):
        p = ac.hand_params(H, W, rects, r1, r2)
        g1, g2, gf, gv = (o[0] for o in ac.run(lib, img[:1], img[1:], flow[None], p, DEV))
        want2 = img[1].astype(np.float32)
        for x0, y0, dx, dy in rects:
            want2[y0:y0 + dy, x0:x0 + dx] = mean
        assert np.array_equal(g1, np.roll(img[0], r1, axis=1).transpose(2, 0, 1)), what
        assert np.array_equal(g2, np.roll(want2, r1 if r2 is None else r2, axis=1).transpose(2, 0, 1)), what
        with np.errstate(invalid="ignore"):
            ref = ar.augment_sample(img[0], img[1], flow, p.row(0))
        assert ac.same_flow(gf, ref[2]) and np.array_equal(gv, ref[3]), what


# ---- bar 6: plumbing --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ac.SIZES, ids=ac.tag)
def test_batch_equals_single_samples_and_repeats_are_identical(lib, gold, size):
    from prior_flow_amd import augment as ag
    i1, i2, fl, p = _mixed_batch(gold, size, 3)
    assert len({tuple(p.words[b]) for b in range(3)}) == 3
    whole = ac.run(lib, i1, i2, fl, p, DEV)
    for b in range(3):
        q = ag.AugmentParams(1)
        q.words[0] = p.words[b]
        one = ac.run(lib, i1[b:b + 1], i2[b:b + 1], fl[b:b + 1], q, DEV)
        assert all(np.array_equal(w[b], o[0], equal_nan=True) for w, o in zip(whole, one)), b
    aug = ag.DeviceAugmentor360(3, *size, DEV)
    ins = (_t(i1), _t(i2), _t(fl))
    first = [o.clone() for o in aug(*ins, p)]
    for _ in range(4):
        again = aug(*ins, p)
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(first, again))
    assert all(np.array_equal(a.cpu().numpy(), w, equal_nan=True) for a, w in zip(first, whole))


def test_out_guard_bands_and_unaligned_bases(lib, gold):
    """out= writes in place; NaN guard bands around every output stay untouched; bases offset by one element (outputs: the
    one-pixel path; inputs: byte loads) give the same bytes."""
    from prior_flow_amd import augment as ag
    size = ac.SIZES[0]
    H, W = size
    B = 2
    i1, i2, fl, p = _mixed_batch(gold, size, B)
    aug = ag.DeviceAugmentor360(B, H, W, DEV, outputs=False)
    with pytest.raises(ag.PfError):
        aug(_t(i1), _t(i2), _t(fl), p)
    want = ac.run(lib, i1, i2, fl, p, DEV)
    shapes = ((B, 3, H, W), (B, 3, H, W), (B, 2, H, W), (B, H, W))
    for off in (64, 65):                                     # floats: 16-byte aligned, then not
        bufs = [torch.full((int(np.prod(s)) + 2 * off + 64,), float("nan"), device=DEV) for s in shapes]
        outs = [b[off:off + int(np.prod(s))].view(s) for b, s in zip(bufs, shapes)]
        ins = []
        for a in (i1, i2, fl):                               # inputs at an odd element offset as well when off is odd
            flat = torch.zeros(a.size + 8, dtype=_t(a).dtype, device=DEV)
            flat[off % 2:off % 2 + a.size] = _t(a).reshape(-1)
            ins.append(flat[off % 2:off % 2 + a.size].view(a.shape))
        got = aug(*ins, p, out=outs)
        assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, outs))
        for b, o, s, w in zip(bufs, outs, shapes, want):
            n = int(np.prod(s))
            assert torch.isnan(b[:off]).all() and torch.isnan(b[off + n:]).all(), off
            assert np.array_equal(o.cpu().numpy(), w, equal_nan=True), off


def test_refusals(lib, gold):
    from prior_flow_amd import augment as ag
    H, W = ac.SIZES[0]
    i1, i2, fl, p = _mixed_batch(gold, (H, W), 1)
    aug = ag.DeviceAugmentor360(1, H, W, DEV)
    good = (_t(i1), _t(i2), _t(fl))
    for bad in ((torch.from_numpy(i1), good[1], good[2]), (good[0].float(), good[1], good[2]), (good[0], good[1], good[2].double()),
                (good[0][:, :-1], good[1], good[2]), (good[0], good[1], good[2].permute(0, 3, 1, 2))):
        with pytest.raises(ag.PfError):
            aug(*bad, p)
    with pytest.raises(ag.PfError):
        aug(*good, ag.AugmentParams(2))
    with pytest.raises(ag.PfError):
        aug(*good, p, out=aug.out[:3])


def test_captured_call_replays_on_new_inputs_and_parameters(lib, gold):
    """A captured call replayed on new inputs and parameters in the same buffers equals the eager call; the caching allocator
    hands out nothing across calls, inside the capture included."""
    from prior_flow_amd import augment as ag
    size = ac.SIZES[1]
    B = 2
    i1, i2, fl, p = _mixed_batch(gold, size, B)
    aug = ag.DeviceAugmentor360(B, *size, DEV)
    ins = [_t(a) for a in (i1, i2, fl)]
    aug(*ins, p)                                             # warm up (module load) before counting
    torch.cuda.synchronize()
    count = lambda: torch.cuda.memory_stats(DEV)["allocation.all.allocated"]  # noqa: E731
    before = count()
    aug(*ins, p)
    aug(*ins)
    assert count() == before
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        graph.capture_begin()
        inside = count()
        aug(*ins)                                            # params=None: the table as it stands on the device
        assert count() == inside
        graph.capture_end()
    torch.cuda.current_stream(DEV).wait_stream(side)
    # new inputs and a new table in the same buffers
    j1, j2, jf, q = _mixed_batch(gold, size, B + 1)
    for dst, src in zip(ins, (j1[1:], j2[1:], jf[1:])):
        dst.copy_(_t(src))
    q2 = ag.AugmentParams(B)
    q2.words[:] = q.words[1:]
    aug.upload(q2)
    for o in aug.out:
        o.fill_(float("nan"))
    graph.replay()
    replayed = [o.clone() for o in aug.out]
    eager = aug(*ins, q2)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(replayed, eager))
    want = ac.run(lib, j1[1:], j2[1:], jf[1:], q2, DEV)
    assert all(np.array_equal(a.cpu().numpy(), w, equal_nan=True) for a, w in zip(replayed, want))
    assert not np.array_equal(want[0], ac.run(lib, i1, i2, fl, p, DEV)[0])


def _feeder_case(gold, n_batches, B=2):
    """Host batches of 64x128, the sampler's keywords, and what direct calls with the same random streams (seed 42) give."""
    from prior_flow_amd import augment as ag
    size = ac.SIZES[0]
    H, W = size
    batches = []
    for k in range(n_batches):
        i1, i2, fl, _ = _mixed_batch(gold, size, B)
        batches.append((torch.from_numpy(np.roll(i1, 7 * k, axis=2).copy()), np.roll(i2, 3 * k, axis=1).copy(),
                        torch.from_numpy(np.roll(fl, k, axis=1).copy()), "extra item"))
    kw = dict(asymmetric_rotaton_aug_prob=0.5, eraser_aug_prob=0.9, rotaton_aug_prob=0.9)
    direct = ag.DeviceAugmentor360(B, H, W, DEV)
    rng, gen = np.random.RandomState(42), torch.Generator().manual_seed(42)
    want = []
    for b in batches:
        p = ag.sample_params_360(B, H, W, rng, gen, **kw)
        want.append([o.clone() for o in direct(_t(np.asarray(b[0])), _t(np.asarray(b[1])), _t(np.asarray(b[2])), p)])
    torch.cuda.synchronize()
    return batches, kw, want, ag.DeviceAugmentor360(B, H, W, DEV, outputs=False)


def _busy(big, n):
    """A few milliseconds of device work on the current stream (n passes over 256 MB), enqueued only: the host runs ahead."""
    for _ in range(n):
        big.mul_(1.0)


def _same(got, want):
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, want))


def test_augmented_batches_equal_direct_calls_without_host_syncs(lib, gold):
    """depth = 2 over six batches yields what six direct calls with the same random streams yield.  The consumer's contract, with
    no host synchronise between the yields: on every set it enqueues a long kernel, a device-side copy of the set and an
    in-place overwrite, then asks for the next batch, so its work on a set is still pending when the feeder prepares that set
    again (the feeder's event, not the host, must order them).  Everything is compared once after the loop."""
    from prior_flow_amd import augment as ag
    batches, kw, want, feeder = _feeder_case(gold, 6)
    big = torch.ones(64 << 20, device=DEV)
    kept = [[torch.empty_like(w) for w in ws] for ws in want]      # allocated up front: no allocation between the yields
    n = 0
    for got in ag.augmented_batches(batches, feeder, np.random.RandomState(42), torch.Generator().manual_seed(42), depth=2, **kw):
        _busy(big, 20)                                       # the consumer's stream stays behind the host
        for dst, g in zip(kept[n], got):
            dst.copy_(g)
        for g in got:
            g.fill_(float("nan"))                            # its in-place use of the set it owns
        n += 1
    torch.cuda.synchronize()
    assert n == 6
    for k in range(6):
        assert _same(kept[k], want[k]), k
    rng, gen = np.random.RandomState(1), torch.Generator().manual_seed(1)
    assert len(list(ag.augmented_batches(batches[:3], feeder, rng, gen, depth=1))) == 3
    with pytest.raises(ag.PfError):
        next(ag.augmented_batches([(batches[0][0].float(),) + batches[0][1:]], feeder, rng, gen))


def test_augmented_batches_start_behind_queued_work(lib, gold):
    """The feeder is started while the current stream has a backlog that still reads a tensor whose block has just gone back to
    the allocator (the feeder's output sets are the same size and are allocated next): the side stream must start behind that
    work, and behind the zero fill of its own outputs.  The pending reader sees its data, and batch 0 is whole."""
    from prior_flow_amd import augment as ag
    batches, kw, want, feeder = _feeder_case(gold, 3)
    big = torch.ones(64 << 20, device=DEV)
    marker = [torch.full_like(w, 7.0) for w in want[0]]
    seen = [torch.empty_like(w) for w in want[0]]
    kept = [[torch.empty_like(w) for w in ws] for ws in want]
    torch.cuda.synchronize()
    _busy(big, 40)
    for dst, m in zip(seen, marker):
        dst.copy_(m)                                         # queued behind the backlog
    del marker, m                                            # the blocks are free for the next allocation on this stream
    n = 0
    for got in ag.augmented_batches(batches, feeder, np.random.RandomState(42), torch.Generator().manual_seed(42), depth=2, **kw):
        for dst, g in zip(kept[n], got):
            dst.copy_(g)
        n += 1
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in seen)
    for k in range(3):
        assert _same(kept[k], want[k]), k


def test_augmented_batches_closed_early(lib, gold):
    """The consumer leaves its loop after the first batch (how train_flow.py's loop ends at num_steps) while the side stream
    still has the batches prepared ahead queued behind a backlog: closing the generator must let them finish before the
    buffers go back to the allocator.  Tensors allocated right afterwards keep their contents."""
    from prior_flow_amd import augment as ag
    batches, kw, want, feeder = _feeder_case(gold, 4)
    big = torch.ones(64 << 20, device=DEV)
    first = [torch.empty_like(w) for w in want[0]]
    torch.cuda.synchronize()
    _busy(big, 40)                                           # the side stream starts behind this
    g = ag.augmented_batches(batches, feeder, np.random.RandomState(42), torch.Generator().manual_seed(42), depth=2, **kw)
    got = next(g)
    for dst, t in zip(first, got):
        dst.copy_(t)
    del got, t
    g.close()
    fresh = [torch.full_like(w, 3.0) for ws in want[:2] for w in ws]      # takes the blocks the feeder gave back
    torch.cuda.synchronize()
    assert all(bool((t == 3.0).all()) for t in fresh)
    assert _same(first, want[0])


def test_odd_shape_takes_the_tail_of_the_contrast_pass(lib):
    """5 x 7: H * W is no multiple of 4, so the contrast pass sums its last pixels in its tail; against the restatement."""
    i1, i2, fl, p = ac.small_odd_batch()
    got = ac.run(lib, i1, i2, fl, p, DEV)
    for b in range(i1.shape[0]):
        with np.errstate(invalid="ignore"):
            want = ar.augment_sample(i1[b], i2[b], fl[b], p.row(b))
        share, worst = ac.image_diff(np.stack([got[0][b], got[1][b]]), np.stack(want[:2]))
        assert share <= ac.CAP_SHARE and worst <= ac.CAP_CHAIN, (b, share, worst)
        assert ac.same_flow(got[2][b], want[2]) and np.array_equal(got[3][b], want[3]), b


def test_large_shape_against_the_restatement(lib):
    """512 x 1024, B = 2: 512 workgroups per plane, below the cap of 1024, so every thread goes round its loop once (the shapes
    at which the loops make a second trip: test_capped_grids_against_the_restatement_and_the_emulation); under bar 2."""
    from prior_flow_amd import augment as ag
    H, W, B = 512, 1024, 2
    r = np.random.RandomState(9)
    i1, i2 = (r.randint(0, 256, (B, H, W, 3)).astype(np.uint8) for _ in range(2))
    fl = np.stack([np.tile(ac.make_flow(64, 128, 40 + b), (8, 8, 1)) * np.float32(4) for b in range(B)])
    p = ag.sample_params_360(B, H, W, np.random.RandomState(3), torch.Generator().manual_seed(3), eraser_aug_prob=1.0,
                             rotaton_aug_prob=1.0, asymmetric_color_aug_prob=1.0)
    p.set_roll(1, -101, 57)
    p.set_asymmetric_colour(0, True).set_asymmetric_colour(1, False)
    got = ac.run(lib, i1, i2, fl, p, DEV)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            w1, w2, wf, wv = ar.augment_sample(i1[b], i2[b], fl[b], p.row(b))
        share, worst = ac.image_diff(np.stack([got[0][b], got[1][b]]), np.stack([w1, w2]))
        print(f"512x1024 sample {b}: share of differing bytes {share:.2e}, worst {worst:.0f}")
        assert share <= ac.CAP_SHARE and worst <= ac.CAP_CHAIN
        assert ac.same_flow(got[2][b], wf) and np.array_equal(got[3][b], wv)


@pytest.mark.parametrize("shape", ac.CAPPED, ids=lambda s: "x".join(map(str, s)))
def test_capped_grids_against_the_restatement_and_the_emulation(lib, emu, shape):
    """The shapes at which pf_aug_blocks caps a grid at 1024 workgroups and its threads make a second trip: (1, 514, 2048), four
    pixels per thread, rows 512 and 513 in the second trip of the main kernel and of the contrast pass, whose sum over those
    rows moves int(mean + 0.5) from 100 to 101 (tests/test_augment_host.py shows it); (2, 258, 1018), one pixel per thread, the
    last 500 pixels; and a rectangle of 12 000 pixels for the 10 240 threads of the eraser.  Under bar 2 against the
    restatement, and equal to the emulation on every byte (no hue step in these chains)."""
    import launch_paths as lp
    B, H, W = shape
    grids = dict(lp.augment_grids(H, W), erase=lp.aug_erase_grid(ac.CAPPED_RECT, H, W))
    print(f"{B}x{H}x{W}: " + ", ".join(f"{k} {g[1]} of {g[0]} wanted, {g[2]} trip(s)" for k, g in grids.items()))
    assert grids["erase"][2] == 2 and [g[2] for k, g in grids.items() if k.startswith("main")] == [2]
    assert grids["contrast"][2] == (2 if H == 514 else 1)
    assert emu is not None
    i1, i2, fl, p, row0 = ac.capped_batch(shape)
    got = ac.run(lib, i1, i2, fl, p, DEV)
    host = ac.run(emu, i1, i2, fl, p)
    for b in range(B):
        with np.errstate(invalid="ignore"):
            w1, w2, wf, wv = ar.augment_sample(i1[b], i2[b], fl[b], p.row(b))
        share, worst = ac.image_diff(np.stack([got[0][b], got[1][b]]), np.stack([w1, w2]))
        print(f"{H}x{W} sample {b}: share of differing bytes {share:.2e}, worst {worst:.0f}")
        assert share <= ac.CAP_SHARE and worst <= ac.CAP_CHAIN
        assert ac.same_flow(got[2][b], wf) and np.array_equal(got[3][b], wv)
    assert all(np.array_equal(g, h, equal_nan=True) for g, h in zip(got, host))
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any() and not np.isnan(got[3]).any()
