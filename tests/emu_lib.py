"""The host emulation library of the per-element kernels (tests/emu/pf_emu.cpp over csrc/pf_elem.h), built and loaded in one
place for every test module that drives it (not a conftest; nothing here is collected).  `__graft_entry__.build_emu` owns the
compiler flags and the staleness check; the entry points the emulation does not have are listed here."""
import os
import shutil

import pytest

# entry points of libpriorflow_hip.so that exist only as device code
EMU_OPTIONAL = ("pf_debug_dirty_lds", "pf_conv2d", "pf_conv2d_tile", "pf_conv2d_stats_blocks", "pf_conv2d_roles", "pf_corr_pyramid",
                "pf_corr_pyramid_bf16x3", "pf_conv2d_wgrad", "pf_dccl_combine_conv1x1", "pf_conv2d_wgrad_small", "pf_conv2d_wgrad_small_ws",
                "pf_conv2d_wgrad_small_ws_floats", "pf_enc_stem")


def load():
    """PfLib over tests/emu/libpf_emu.so, rebuilt when a source is newer; skips the calling test where there is no g++ and no
    library from an earlier build."""
    import __graft_entry__ as ge
    from prior_flow_amd._lib import PfLib
    so = ge.build_emu()
    if not os.path.exists(so):
        pytest.skip("g++ not available" if shutil.which("g++") is None else "the host emulation did not build")
    return PfLib(so, require_cuda=False, optional=EMU_OPTIONAL)
