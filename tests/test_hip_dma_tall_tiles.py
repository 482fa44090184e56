"""The 256-pixel tiles of the 3x3 all-DMA convolutions on the device: pf_conv_dma_kernel<1,3,3,1> (256 px x 32 channels, new) and
<2,3,3,1> where the planner's byte rule now takes it (csrc/pf_conv_api.hip: conv_dma_tile_3x3).

Every case of run_tall_tile_case.CASES runs in two child processes (PRIORFLOW_DMA_TALL is read once per process): with the rule,
and with PRIORFLOW_DMA_TALL=0 on the tile the planner took before.  Each child checks its outputs against float64 under the
bounds of conv_launches.py, sentinels included; the two children's outputs must be equal bit for bit, because every tile of this
kernel keeps the same MFMA order per accumulator -- a difference is a bug in the new tile, not a rounding question."""
import os
import subprocess
import sys

import pytest
import torch

import run_tall_tile_case as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("tall_tiles")
    out = {}
    for tag, knob in (("rule", "1"), ("before", "0")):
        path = str(tmp / f"{tag}.pt")
        env = dict(os.environ, PRIORFLOW_DMA_TALL=knob)
        p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "run_tall_tile_case.py"), path],
                           env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
        print(f"--- PRIORFLOW_DMA_TALL={knob}\n{p.stdout.decode(errors='replace')}")
        assert p.returncode == 0, f"child with PRIORFLOW_DMA_TALL={knob} ended with {p.returncode}"
        out[tag] = torch.load(path)
    return out


@pytest.mark.parametrize("name", list(rc.CASES))
def test_tall_tile_matches_fp64_and_the_tile_before_bitwise(runs, name):
    want_rule, want_before = rc.CASES[name][-2:]
    rule, before = runs["rule"][name], runs["before"][name]
    assert tuple(rule["plan"]) == want_rule and tuple(before["plan"]) == want_before, (rule["plan"], before["plan"])
    assert not rule["fails"], rule["fails"]
    assert not before["fails"], before["fails"]
    assert rule["outs"].keys() == before["outs"].keys() and rule["outs"]
    for key, got in rule["outs"].items():
        ref = before["outs"][key]
        assert torch.equal(got.view(torch.uint8), ref.view(torch.uint8)), \
            (key, int((got.view(torch.uint8) != ref.view(torch.uint8)).sum()), "bytes differ from the 128-pixel tile's")
