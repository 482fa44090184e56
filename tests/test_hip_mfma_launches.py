"""The matrix-core kernels outside pf_conv2d -- the correlation build on each of its launcher paths, the operand splits, the
feature pyramid and the encoders' stem -- on libpriorflow_hip.so against float64 under derived bounds (tests/mfma_launches.py:
cases, references, bounds), one test per (family, shape).  The default kernels run in this process; PRIORFLOW_CORR_RS, which the
launcher reads per launch, is the only switch touched, for the cases that need the tile kernel on a map the role-split kernel
would take.  The float64 references run in torch on the device.  The table printed at the end -- kernel and path, shape, worst
|err| / bound -- is the one DESIGN.md quotes next to the emulations'."""
import time

import pytest
import torch

import mfma_launches as ml

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from prior_flow_amd import _lib
    return _lib.load()          # raises if the HIP library was not built: no fallback


@pytest.fixture(scope="module")
def table():
    t = ml.Table()
    yield t
    print("\nMI355X, worst |err| / bound\n" + t.render())


@pytest.fixture(scope="module")
def paths():
    return set()


@pytest.mark.parametrize("family,shape", ml.cases("gpu"), ids=lambda v: str(v))
def test_launch_matches_float64(lib, table, paths, family, shape, monkeypatch, capsys):
    dev = torch.device("cuda:0")
    monkeypatch.delenv("PRIORFLOW_CORR_RS", raising=False)
    for k, v in ml.case_env(family, shape).items():
        monkeypatch.setenv(k, v)
    t0 = time.time()
    fails = ml.run_case(lib, family, shape, dev, table, paths)
    torch.cuda.synchronize()
    with capsys.disabled():
        print(f" [{family} {shape}: {time.time() - t0:.1f} s]", end="")
    assert not fails, "\n".join(fails)


def test_every_corr_path_ran(paths):
    """Runs after the cases above: every (kernel path, RB, chunks, precision, scale branch) the launcher can select was launched."""
    assert ml.selectable_corr_paths() <= paths, sorted(ml.selectable_corr_paths() - paths)
