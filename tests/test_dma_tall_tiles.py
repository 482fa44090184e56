"""The tile choice of the 3x3 all-DMA convolutions (csrc/pf_conv_api.hip: dma_tile_cost, conv_dma_tile_3x3): host logic over
fake pointers, as in test_abi.py.  No GPU.

The 256-pixel tiles stage fewer bytes per K-step than the 128-pixel ones, and the planner takes the tile
whose busiest workgroup stages the fewest.  PRIORFLOW_DMA_TALL=0 restores the choices of the commit before the rule; it is read
once per process, so that side runs in a child.  tests/golden/conv_plans_before_tall_tiles.json holds what that commit's
library answered over the sweep below (`python tests/test_dma_tall_tiles.py OUT.json` with PRIORFLOW_LIB naming that library)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv_plans_before_tall_tiles.json")
FAKE = 0x1000

# the grid of test_abi.py::test_plan_invariants_over_product_launches, and the same launches as one chain of two (co_groups 1)
FORMS = ((0, "fp32"), (1, "fp32"), (1, "split"), (2, "split"))
CONVS = ((64, 64, 3, 3, 1), (96, 96, 3, 3, 1), (128, 256, 3, 3, 1), (256, 128, 1, 5, 1), (256, 384, 5, 1, 1), (256, 2, 1, 1, 1),
         (128, 64, 4, 4, 1), (64, 96, 3, 3, 2), (96, 128, 1, 1, 2),
         # the update blocks' 3x3 launches this rule is about
         (256, 128, 3, 3, 1), (272, 126, 3, 3, 1), (256, 192, 3, 3, 1), (128, 64, 3, 3, 1))
GEOS = ((1, 64, 128), (2, 32, 64), (4, 256, 512), (8, 64, 128), (32, 64, 128), (1, 80, 160), (1, 37, 53))
GROUPS = ((1, 0), (2, 0), (1, 1), (3, 0))          # (groups of the launch, co_groups)


def _lib():
    import __graft_entry__ as ge
    ge.build_hip()
    from prior_flow_amd import _lib
    return _lib.PfLib(_lib.LIB_PATH, require_cuda=False)


def _desc(cin, cout, kh, kw, prec=1, form="split", stride=1, co=0):
    from prior_flow_amd import _lib
    d = _lib.ConvDesc()
    cpc = 64 if prec == _lib.PREC_F16 else 32
    if form == "fp32":
        d.in0, d.ld0 = FAKE, cin
    else:
        d.in0_split, d.lds0 = FAKE, (cin + cpc - 1) // cpc
        d.zeros, d.zeros_bytes = FAKE, 4096
    d.c0, d.weight, d.bias = cin, FAKE, FAKE
    d.out, d.ld_out, d.cout = FAKE, cout, cout
    d.kh, d.kw, d.stride, d.epilogue, d.scale, d.precision = kh, kw, stride, _lib.EPI_RELU, 1.0, prec
    d.co_groups = co
    return d


def _plan(lib, ds, B, H, W):
    from prior_flow_amd import _lib
    a = (_lib.ConvDesc * len(ds))(*ds)
    return [int(f(a, len(ds), B, H, W)) for f in (lib._dll.pf_conv2d_tile, lib._dll.pf_conv2d_roles, lib._dll.pf_conv2d_stats_blocks)]


def sweep(lib):
    """[[key, [tile, roles, stats blocks]], ...] over FORMS x CONVS x GEOS x GROUPS, in that order."""
    out = []
    for prec, form in FORMS:
        for cin, cout, kh, kw, stride in CONVS:
            for B, H, W in GEOS:
                for ng, co in GROUPS:
                    ds = [_desc(cin, cout, kh, kw, prec, form, stride, co) for _ in range(ng)]
                    out.append([[prec, form, cin, cout, kh, kw, stride, B, H, W, ng, co], _plan(lib, ds, B, H, W)])
    return out


@pytest.fixture(scope="module")
def lib():
    return _lib()


@pytest.fixture(scope="module")
def before():
    return {tuple(k): v for k, v in json.load(open(GOLDEN))}


def test_update_block_launches_take_the_256_pixel_tiles(lib):
    """One 512 x 1024 pair, split operands: as one chain of two (co_groups 1) and as one launch of two groups, 256 -> 128 and
    272 -> 126 take 256 px x 32 channels (tile 3, roles 18), 256 -> 192 takes 256 px x 64 channels (tile 4, roles 18)."""
    for cin, cout, want in ((256, 128, [3, 18]), (272, 126, [3, 18]), (256, 192, [4, 18])):
        one = _plan(lib, [_desc(cin, cout, 3, 3, co=1)], 1, 64, 128)
        two = _plan(lib, [_desc(cin, cout, 3, 3), _desc(cin, cout, 3, 3)], 1, 64, 128)
        assert one[:2] == want and two[:2] == want, (cin, cout, one, two)
    # the three 64-channel convolutions of the flow chain as one launch: 192 items either way, 8.9 KB per step instead of 11.1
    assert _plan(lib, [_desc(128, 64, 3, 3) for _ in range(3)], 1, 64, 128)[:2] == [3, 18]
    # 128 -> 256 (the FlowHead stem) keeps 256 px x 64 channels: 128 items in one round against 256 items of 32 channels in two
    assert _plan(lib, [_desc(128, 256, 3, 3, co=1)], 1, 64, 128)[:2] == [4, 18]
    # f16 maps follow the same rule (the bytes per row are the same)
    assert _plan(lib, [_desc(256, 128, 3, 3, prec=2, co=1)], 1, 64, 128)[:2] == [3, 18]


def test_partial_tiles_count_as_items(lib):
    """A 12-row map has two 8-row tiles (one half empty) against three 4-row tiles: 4/3 of the items.  Where every candidate
    still fits its share of the chip in one round, the lighter K-step decides; where the extra items cost a second round,
    they lose."""
    # 2 images of 12 x 40, two groups of 126 channels: 48 items of 128 px x 64 or 64 items of 256 px x 32, one round both
    assert _plan(lib, [_desc(96, 126, 3, 3), _desc(96, 126, 3, 3)], 2, 12, 40)[:2] == [3, 18]
    # 20 images of 12 x 32 in four groups of 64 channels: 240 items of 128 px x 64 (one round at 11.1 KB) against 320 items of
    # 256 px x 32 (two rounds at 8.9 KB) and 160 of 256 px x 64 (one round at 12.9 KB): the 128-pixel tile stays
    assert _plan(lib, [_desc(96, 64, 3, 3) for _ in range(4)], 20, 12, 32)[:2] == [3, 17]


def test_a_launch_alone_on_the_chip_and_other_shapes_keep_their_plans(lib, before):
    """One group without co_groups, every 1x5 / 5x1 / 1x1 / 4x4 / stride-2 launch and every fp32-operand launch plan as before."""
    n = 0
    for key, got in sweep(lib):
        prec, form, cin, cout, kh, kw, stride, B, H, W, ng, co = key
        if (kh, kw) != (3, 3) or stride != 1 or form != "split" or (ng == 1 and co == 0):
            assert got == before[tuple(key)], (key, got, before[tuple(key)])
            n += 1
        elif got[0] >= 0:
            assert got[1] in (17, 18) and got[0] in (3, 4, 5, 8), (key, got)
            if before[tuple(key)][0] in (5, 8):          # the big-map tiles are not this rule's
                assert got == before[tuple(key)], (key, got)
    assert n > 1000


def test_knob_off_restores_every_plan(lib, before):
    """PRIORFLOW_DMA_TALL=0 in a fresh process: the whole sweep equals the recorded plans of the commit before the rule."""
    env = dict(os.environ, PRIORFLOW_DMA_TALL="0")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "-"], stdout=subprocess.PIPE, env=env, check=True, timeout=300)
    got = json.loads(p.stdout.decode())
    assert len(got) == len(before) == len(FORMS) * len(CONVS) * len(GEOS) * len(GROUPS)
    diff = [(k, v, before[tuple(k)]) for k, v in got if v != before[tuple(k)]]
    assert not diff, diff[:10]


def test_the_default_differs_from_the_knob_off_plans_only_by_the_tile(lib, before):
    """With the rule on, a 3x3 launch either keeps its plan or moves between tiles of the same kernel; the sweep sees both new
    choices (256 px x 32 channels where 128 px x 64 was, 256 px x 64 where 128 px x 128 was)."""
    moved = set()
    for key, got in sweep(lib):
        was = before[tuple(key)]
        if got != was:
            assert was[1] in (17, 18) and got[1] in (17, 18) and got[2] == was[2], (key, got, was)
            moved.add((tuple(was[:2]), tuple(got[:2])))
    assert ((3, 17), (3, 18)) in moved and ((4, 17), (4, 18)) in moved, moved


def test_the_device_cases_are_planned_as_their_table_says(lib):
    """run_tall_tile_case.CASES (the launches test_hip_dma_tall_tiles.py runs on the device) name the plan each takes with the
    rule: host logic, checked here so that a planner change cannot quietly turn the device test into a test of another tile."""
    import conv_launches as cl
    import run_tall_tile_case as rc
    for name, spec in rc.CASES.items():
        ln = rc.launch_of(lib, name)
        assert cl.plan(lib, cl.fake_descs(ln), ln.B, ln.H, ln.W) == spec[-2], name


if __name__ == "__main__":                      # the sweep as JSON, on the library _lib.LIB_PATH names: to a file, or "-" for stdout
    sys.path.insert(0, os.path.dirname(HERE))
    from prior_flow_amd import _lib as L
    text = json.dumps(sweep(L.PfLib(L.LIB_PATH, require_cuda=False)))
    if sys.argv[1] == "-":
        sys.stdout.write(text)
    else:
        open(sys.argv[1], "w").write(text + "\n")
