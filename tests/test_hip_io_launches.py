"""The launches before the encoders and after the last iteration -- sample grid, input stage, evaluation metrics and region sums,
weight pack / batched pack / unpack, layout plumbing -- on libpriorflow_hip.so against float64 under derived bounds
(tests/io_launches.py: cases, references, bounds), one test per (kernel family, shape).  The default kernels are the ones under
test: no environment switch, no child process.  The float64 references run in torch on the device (numpy for the bit-exact weight
packs).  The table printed at the end -- kernel, shape, worst |err| / bound -- is the one DESIGN.md quotes next to the host
emulation's."""
import pytest
import torch

import io_launches as io

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd import _lib
    return _lib.load()          # raises if the HIP library was not built: no fallback


@pytest.fixture(scope="module")
def table():
    t = io.Table()
    yield t
    print("\nMI355X, worst |err| / bound\n" + t.render())


@pytest.mark.parametrize("family,shape", io.cases("gpu"), ids=lambda v: str(v))
def test_launch_matches_float64(lib, table, family, shape):
    dev = torch.device("cuda:0")
    fails = io.run_case(lib, family, shape, dev, table)
    torch.cuda.synchronize()
    assert not fails, "\n".join(fails[:40])
