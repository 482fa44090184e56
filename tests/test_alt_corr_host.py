"""alternate_corr without a GPU: the C-ABI declares and exports the two entry points, the host emulation of their element
forms (csrc/pf_elem.h: pf_feat_pool_elem, pf_lookup_feat_elem) equals the oracle's lookups in the volume pyramid up to
rounding, and both builds refuse bad arguments before any launch."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

import alt_corr_ref as ref
import golden_cases as gc
import priorflow_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_SO = os.path.join(EMU_DIR, "libpf_emu.so")
CSRC = os.path.join(ROOT, "prior-flow_amd", "csrc")
EPS = float(torch.finfo(torch.float32).eps)
NEW = ("pf_feature_pyramid", "pf_dccl_lookup_feat")


@pytest.fixture(scope="module")
def emu():
    """The host emulation library, built as tests/test_emu_kernels.py builds it."""
    import emu_lib
    return emu_lib.load()


def test_header_and_exports_declare_the_entry_points():
    text = open(os.path.join(ROOT, "include", "priorflow_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared"
    from prior_flow_amd import _lib
    assert set(NEW) <= set(_lib.EXPORTS)


def test_emulation_exports_the_entry_points(emu):
    for name in NEW:
        assert hasattr(emu._dll, name), f"the emulation build does not export {name}"


def _case(tag, B, h, w):
    f1a, f2a = gc.fmaps(tag + "/a", B, h, w)
    f1b, f2b = gc.fmaps(tag + "/b", B, h, w)
    coords = gc.nasty_coords(tag, B, h, w)
    g = po.sample_grid(h, w, po.rotation_x(math.pi / 2)).contiguous()     # branch A: grid(R_B2A) both ways
    return f1a, f2a, f1b, f2b, coords, g


def _levels(lib, f2, B, h, w):
    rows = ref.rows(f2)
    lv = [torch.empty(B * (h >> i) * (w >> i), f2.shape[1]) for i in (1, 2, 3)]
    lib.feature_pyramid(rows, lv, B, h, w)
    return [rows] + lv


def _uncl(x, B, h, w):
    return x[:, :324].reshape(B, h, w, 324).permute(0, 3, 1, 2)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("hw", [(16, 32), (20, 44), (16, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_emulated_lookup_feat_matches_oracle(emu, hw, B):
    h, w = hw
    f1a, f2a, f1b, f2b, coords, g = _case(f"altcorr/{h}x{w}/{B}", B, h, w)
    C = f1a.shape[1]
    # pooled features: the oracle's floor 2x2 means, level by level
    lv_a = _levels(emu, f2a, B, h, w)
    for i, want in enumerate(ref.pool_levels(f2a.double())):
        bound = 3 * (i + 1) * EPS * ref.pool_levels(f2a.double().abs())[i]
        assert bool(((ref.rows(want) - lv_a[i].double()).abs() <= ref.rows(bound)).all()), f"level {i}"
    lv_b = _levels(emu, f2b, B, h, w)
    own = torch.full((B * h * w, 324), 7.0)
    raw = torch.full((B * h * w, 324), 7.0)
    emu.dccl_lookup_feat(coords, ref.rows(f1a), lv_a, ref.rows(f1b), lv_b, g, own, raw)
    # the oracle on the volumes: own directly, own + cross through pf_dccl_combine
    o_own, o_cross = po.dccl_lookup(coords, po.build_pyramid(po.corr_volume(f1a, f2a)),
                                    po.build_pyramid(po.corr_volume(f1b, f2b)), g, g)
    m_own, m_raw = ref.lookup_feat(coords, f1a, f2a, f1b, f2b, g, absolute=True)
    m_own = _uncl(m_own, B, h, w)
    m_cross = po.img_rotate(_uncl(m_raw, B, h, w), g)
    # worst case of both sides' fp32 sums (C-term dot products, pooling, bilinear weights): (C + 32) eps x the magnitude
    k = (C + 32) * EPS
    err = (_uncl(own, B, h, w).double() - o_own.double()).abs()
    assert bool((err <= k * m_own).all()), f"own: worst err / bound {float((err / (k * m_own + 1e-30)).max()):.3g}"
    out = torch.empty(B * h * w, 324)
    emu.dccl_combine(own, raw, g, out, B, h, w)
    err = (_uncl(out, B, h, w).double() - (o_own + o_cross).double()).abs()
    assert bool((err <= k * (m_own + m_cross)).all()), f"own + cross: worst err / bound {float((err / (k * (m_own + m_cross))).max()):.3g}"
    # the data are not trivially inside the bound: the two views differ by far more than it
    assert float((o_own - o_cross).abs().max()) > 1e3 * k * float(m_own.max())


def test_emulated_lookup_feat_matches_float64_restatement(emu):
    """raw (before the rotate-back) row by row against the float64 restatement the GPU tests use."""
    B, h, w = 2, 20, 44
    f1a, f2a, f1b, f2b, coords, g = _case("altcorr/raw", B, h, w)
    own = torch.empty(B * h * w, 324)
    raw = torch.empty(B * h * w, 324)
    emu.dccl_lookup_feat(coords, ref.rows(f1a), _levels(emu, f2a, B, h, w), ref.rows(f1b), _levels(emu, f2b, B, h, w), g, own, raw)
    w_own, w_raw = ref.lookup_feat(coords, f1a, f2a, f1b, f2b, g)
    m_own, m_raw = ref.lookup_feat(coords, f1a, f2a, f1b, f2b, g, absolute=True)
    k = (f1a.shape[1] + 32) * EPS
    assert bool(((own.double() - w_own).abs() <= k * m_own).all())
    assert bool(((raw.double() - w_raw).abs() <= k * m_raw).all())


def _validation(dll):
    f = torch.zeros(16 * 64 * 256 + 16)
    p = ctypes.c_void_p(f.data_ptr())
    odd = ctypes.c_void_p(f.data_ptr() + 4)                 # not 16-byte aligned
    ok = dict(B=1, H8=16, W8=32, C=256, ld=324)

    def look(coords=p, f1=p, own=p, raw=ctypes.c_void_p(f.data_ptr() + 64), own_l2=p, oth_l3=p, **kw):
        a = dict(ok, **kw)
        return dll.pf_dccl_lookup_feat(coords, f1, p, p, own_l2, p, p, p, p, p, oth_l3, p, own, raw, None,
                                       a["B"], a["H8"], a["W8"], a["C"], a["ld"], None)
    assert look(coords=None) == -1                          # PF_ERR_BAD_ARG
    assert look(f1=None) == -1
    assert look(own=None) == -1
    assert look(raw=p) == -1                                # own_out == raw_out
    assert look(f1=odd) == -1
    assert look(ld=323) == -2                               # PF_ERR_BAD_SHAPE
    for C in (0, 6, 1024):
        assert look(C=C) == -2, C
    assert look(H8=15) == -2                                # level 3 would be 1 x 4
    assert look(W8=8) == -2
    assert look(B=0) == -2
    assert look(C=516) == -2                                # one float4 past the two channel groups a lane holds
    assert look(own_l2=odd) == -1 and look(oth_l3=odd) == -1        # a misaligned pooled level of either view
    assert look(own_l2=None) == -1 and look(oth_l3=None) == -1

    def pyr(f2=p, l1=p, **kw):
        a = dict(ok, **kw)
        return dll.pf_feature_pyramid(f2, l1, p, p, a["B"], a["H8"], a["W8"], a["C"], None)
    assert pyr(f2=None) == -1
    assert pyr(l1=None) == -1
    assert pyr(l1=odd) == -1
    assert pyr(C=6) == -2
    assert pyr(H8=8) == -2


def test_argument_validation_emulation(emu):
    _validation(emu._dll)


def test_wrappers_refuse_levels_that_do_not_fit(emu):
    """The typed wrappers check every feature level's rows against B, H8, W8 before the kernels read them."""
    from prior_flow_amd._lib import PfError
    B, h, w, C = 1, 16, 32, 256
    f1a, f2a, f1b, f2b, coords, g = _case("altcorr/shapes", B, h, w)
    lv_a, lv_b = _levels(emu, f2a, B, h, w), _levels(emu, f2b, B, h, w)
    own, raw = torch.empty(B * h * w, 324), torch.empty(B * h * w, 324)
    short = [lv_a[0], lv_a[1][:-1], lv_a[2], lv_a[3]]
    with pytest.raises(PfError, match="feature level 1"):
        emu.dccl_lookup_feat(coords, ref.rows(f1a), short, ref.rows(f1b), lv_b, g, own, raw)
    with pytest.raises(PfError, match="feature level 0"):
        emu.dccl_lookup_feat(coords, ref.rows(f1a), lv_a, ref.rows(f1b), [lv_b[0][:, :128].contiguous()] + lv_b[1:], g, own, raw)
    with pytest.raises(PfError, match="feature level 2"):
        emu.feature_pyramid(ref.rows(f2a), [lv_a[1], lv_a[2][:1], lv_a[3]], B, h, w)


def test_argument_validation_hip_library():
    """The same refusals from the gfx950 library: validation runs before any launch, so no GPU is needed."""
    import __graft_entry__ as ge
    path = ge.build_hip()
    from prior_flow_amd import _lib
    lib = _lib.PfLib(path, require_cuda=False)
    _validation(lib._dll)
