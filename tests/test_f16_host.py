"""Host logic of the fp16 update blocks (mixed_precision, PF_PREC_F16): which kernel an F16 launch takes and which F16
descriptors are refused is arithmetic over the descriptor (pf_conv2d_roles / pf_conv2d_tile launch nothing), and the weight
packing is torch on the CPU.  No GPU needed."""
import argparse

import pytest
import torch

ERR = 0                         # every PF_ERR_* code is negative
FAKE = 0x1000                   # never dereferenced by the planning calls


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_hip()
    from prior_flow_amd import _lib
    return _lib.PfLib(_lib.LIB_PATH, require_cuda=False)


def desc(cin, cout, kh, kw, epi=None, c1=0, precision=None, lds0=None, **fields):
    """F16 descriptor with f16-map operands: in0 = [rows][ceil(c0 / 64) * 64], in1 (c1 > 0) at channel 128 of a 256-wide map."""
    from prior_flow_amd import _lib
    d = _lib.ConvDesc()
    c0 = cin - c1
    d.in0_split, d.lds0, d.off0, d.c0 = FAKE, (c0 + 63) // 64 if lds0 is None else lds0, 0, c0
    if c1:
        d.in1_split, d.lds1, d.off1, d.c1 = FAKE, 4, 128, c1
    d.zeros, d.zeros_bytes = FAKE, 4096
    d.weight, d.bias = FAKE, FAKE
    d.out, d.ld_out, d.off_out, d.cout = FAKE, 512, 0, cout
    d.kh, d.kw = kh, kw
    d.epilogue, d.scale, d.stride = _lib.EPI_RELU if epi is None else epi, 1.0, 1
    d.precision = _lib.PREC_F16 if precision is None else precision
    for name, v in fields.items():
        setattr(d, name, v)
    return d


def arr(*ds):
    from prior_flow_amd import _lib
    return (_lib.ConvDesc * len(ds))(*ds), len(ds)


def roles(lib, ds, B=1, H8=64, W8=128):
    a, n = arr(*ds)
    return lib._dll.pf_conv2d_roles(a, n, B, H8, W8)


def update_block_geometries():
    """Every pf_conv2d launch of the update blocks in f16 mode (engine.py: motion encoders, conv_A / conv, hoisted context,
    SepConvGRU, FlowHead / mask stems), as (name, [descriptors of one launch])."""
    from prior_flow_amd import _lib
    gru_zr = lambda kh, kw: desc(256, 256, kh, kw, _lib.EPI_GRU_ZR, c1=128, h=FAKE, ld_h=128, aux_split=FAKE, lds_aux=2,  # noqa: E731
                                 pre=FAKE, ld_pre=384, off_pre=0)
    gru_q = lambda kh, kw: desc(256, 128, kh, kw, _lib.EPI_GRU_Q, c1=128, h=FAKE, ld_h=128, z=FAKE, ld_z=128,  # noqa: E731
                                out_split=FAKE, lds_out=2, pre=FAKE, ld_pre=384, off_pre=256)
    return [
        ("convc2 A|B", [desc(256, 128, 3, 3, out_split=FAKE, lds_out=5), desc(256, 192, 3, 3, out_split=FAKE, lds_out=5)]),
        ("convf2", [desc(128, 64, 3, 3, out_split=FAKE, lds_out=5, off_out=128)] * 3),
        ("conv_A|conv", [desc(272, 124, 3, 3, out_split=FAKE, lds_out=4, off_out=128),
                         desc(272, 126, 3, 3, out_split=FAKE, lds_out=4, off_out=128)]),
        ("hoisted context 1x5", [desc(128, 384, 1, 5, _lib.EPI_LINEAR, lds0=4)] * 2),
        ("hoisted context 5x1", [desc(128, 384, 5, 1, _lib.EPI_LINEAR, lds0=4)] * 2),
        ("gru zr 1x5", [gru_zr(1, 5)] * 2), ("gru zr 5x1", [gru_zr(5, 1)] * 2),
        ("gru q 1x5", [gru_q(1, 5)] * 2), ("gru q 5x1", [gru_q(5, 1)] * 2),
        ("flow_head.conv1|mask.0", [desc(128, 256, 3, 3)] * 2),
        ("flow_head.conv1 alone", [desc(128, 256, 3, 3)]),
    ]


@pytest.mark.parametrize("B,H8,W8", [(1, 64, 128), (2, 32, 64), (32, 64, 128), (1, 37, 53)])
def test_update_block_geometries_take_the_all_dma_kernel(lib, B, H8, W8):
    seen = set()
    for name, ds in update_block_geometries():
        r = roles(lib, ds, B, H8, W8)
        assert r in (17, 18), (name, r)
        a, n = arr(*ds)
        assert lib._dll.pf_conv2d_tile(a, n, B, H8, W8) >= 3, name
        seen.add(r)
    if (B, H8, W8) == (1, 64, 128):
        assert seen == {17, 18}, seen          # both roles: the 128-px tile and the 256 px x 64 channel tile


def test_co_groups_hint_applies_to_f16(lib):
    one = desc(256, 128, 3, 3)
    one.co_groups = 1
    assert roles(lib, [one]) == roles(lib, [desc(256, 128, 3, 3), desc(256, 192, 3, 3)])


def test_f16_mixed_with_bf16x3_groups_is_refused(lib):
    from prior_flow_amd import _lib
    bf = desc(256, 128, 3, 3, precision=_lib.PREC_BF16X3, lds0=8)
    assert roles(lib, [desc(256, 128, 3, 3), bf]) < ERR
    assert roles(lib, [bf, desc(256, 128, 3, 3)]) < ERR


def test_misaligned_f16_segments_are_refused(lib):
    from prior_flow_amd import _lib
    assert roles(lib, [desc(128, 64, 3, 3, lds0=4, off0=32)]) < ERR             # off0 % 64 != 0 (fine for a twin)
    d = desc(256, 256, 1, 5, _lib.EPI_GRU_ZR, c1=128, h=FAKE, ld_h=128, aux_split=FAKE, lds_aux=2)
    d.off1 = 96                                                                  # off1 % 64 != 0
    assert roles(lib, [d]) < ERR
    d = desc(256, 256, 1, 5, _lib.EPI_GRU_ZR, c1=160, h=FAKE, ld_h=128, aux_split=FAKE, lds_aux=2)
    d.off1 = 64                                                                  # c0 = 96 with a second segment
    assert roles(lib, [d]) < ERR
    # a last segment that ends inside a 64-channel unit must end at its row's end: 272 channels in a 320-wide map, not 384
    assert roles(lib, [desc(272, 124, 3, 3)]) in (17, 18)
    assert roles(lib, [desc(272, 124, 3, 3, lds0=6)]) < ERR
    assert roles(lib, [desc(272, 124, 3, 3, lds0=4)]) < ERR                     # map too narrow
    # the same misaligned offsets are legal for bf16x3 twins (32-channel chunks): only F16 refuses them
    assert roles(lib, [desc(128, 64, 3, 3, precision=_lib.PREC_BF16X3, lds0=8, off0=32)]) in (17, 18)


def test_f16_where_the_all_dma_kernel_does_not_go_is_refused(lib):
    from prior_flow_amd import _lib
    assert roles(lib, [desc(256, 256, 1, 1)]) < ERR                              # 1x1 (mask.2 stays bf16x3)
    assert roles(lib, [desc(64, 64, 7, 7)]) < ERR                                # 7x7
    assert roles(lib, [desc(128, 128, 3, 3, stride=2)], H8=32, W8=64) < ERR       # stride 2
    assert roles(lib, [desc(128, 128, 3, 3, stats_out=FAKE)]) < ERR              # fused statistics
    assert roles(lib, [desc(128, 128, 3, 3, in_scale=FAKE, in_shift=FAKE)]) < ERR
    d = desc(128, 128, 3, 3)
    d.in0_split, d.in0, d.ld0 = None, FAKE, 128                                  # fp32 operands
    assert roles(lib, [d]) < ERR
    for fn in (lib._dll.pf_conv2d_tile, lib._dll.pf_conv2d_stats_blocks):
        a, n = arr(desc(256, 256, 1, 1))
        assert fn(a, n, 1, 64, 128) < ERR
    # precision 3 does not exist
    assert roles(lib, [desc(128, 64, 3, 3, precision=3)]) < ERR


def test_f16_packing_follows_the_declared_set():
    """pack_update_blocks(PREC_F16): exactly the convolutions of engine.F16_CONVS get fp16 weights [Cout_pad][taps][Cin_pad64]
    equal to weight.half(); convc1 and mask.2 keep the bf16x3 packing."""
    from prior_flow_amd import _lib
    from prior_flow_amd.engine import F16_CONVS, Conv, pack_update_blocks
    from prior_flow_amd.modules import state_dict_shapes
    from prior_flow_amd.prior_raft import PriOr_RAFT
    from prior_flow_amd.synthetic import det_state_dict
    m = PriOr_RAFT(argparse.Namespace(mixed_precision=True, dropout=0.0))
    sd = det_state_dict(state_dict_shapes())
    m.load_state_dict(sd, strict=True)
    P = pack_update_blocks(m.ODDC, m.update_block, _lib.PREC_F16)
    assert P["precision"] == _lib.PREC_F16
    convs = {k: v for k, v in P.items() if isinstance(v, Conv)}
    f16 = {k for k, v in convs.items() if v.precision == _lib.PREC_F16}
    assert {k for k, v in convs.items() if v.precision == _lib.PREC_BF16X3} == {"a.c1", "b.c1", "a.m2", "b.m2"}
    assert f16 == set(convs) - {"a.c1", "b.c1", "a.m2", "b.m2"}
    for k in f16:
        w = convs[k].w
        assert w.dtype == torch.float16 and w.shape[-1] % 64 == 0 and w.shape[0] % 128 == 0, k
    # one weight against the reference parameter it packs: conv_A, 272 input channels -> 320
    wa = sd["ODDC.encoder.conv_A.weight"]
    got = convs["a.out"].w
    assert got.shape == (128, 9, 320)
    assert torch.equal(got[:wa.shape[0], :, :272], wa.permute(0, 2, 3, 1).reshape(wa.shape[0], 9, 272).half())
    assert not got[:, :, 272:].any() and not got[wa.shape[0]:].any()
    # the declared set names reference parameters, and F16_CONVS covers what the packing turned into fp16
    names = {k[:-len(".weight")] for k in sd if k.endswith(".weight")}
    assert set(F16_CONVS) <= names
    assert {n for n in F16_CONVS if n.startswith("ODDC.gru.")} == {f"ODDC.gru.conv{g}{t}" for g in "zrq" for t in "12"}
    # the module resolves the flag to the mode, and model.precision overrides it
    assert m._update_precision() == _lib.PREC_F16
    m.precision = _lib.PREC_BF16X3
    assert m._update_precision() == _lib.PREC_BF16X3
