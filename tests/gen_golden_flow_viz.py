"""Emit tests/golden/flow_viz.npz and flow_viz_warp.npz: the reference's colour coding and cyclic warp on stored flows.

Run only where the reference tree is present:  ``python tests/gen_golden_flow_viz.py``.  The fixture holds data only: the
flows and images (tests/flow_viz_cases.py) and what the reference's ``omniflow_to_image``, ``flow_to_image``,
``calculate_veclen_spherical`` and ``my_cycle_warp`` return for them.  Two files, each below 1 MiB, 1.5 MB together: the flows are
fp16-exact and stored as fp16; only 64x128 carries a second image; the warp (flow_viz_warp.npz: the integer-valued image and
my_cycle_warp of it under the first image's flow) is stored at all three sizes, with one channel instead of three at 128x256
(flow_viz_cases.py).  Inert shims on top of
oracle/_refharness.py: a stub ``cv2`` (flow_viz.py imports it for the GIF text overlay only).
"""
from __future__ import annotations

import importlib
import os
import sys
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [_HERE, os.path.join(os.path.dirname(_HERE), "oracle")]

import flow_viz_cases as fc  # noqa: E402
from _refharness import load_reference  # noqa: E402


@torch.no_grad()
def main():
    load_reference()
    cv2 = types.ModuleType("cv2")
    cv2.setNumThreads = lambda n: None
    cv2.ocl = types.SimpleNamespace(setUseOpenCL=lambda b: None)
    sys.modules.setdefault("cv2", cv2)
    fv = importlib.import_module("core.utils.flow_viz")
    sph = importlib.import_module("core.utils.spherical")
    cyc = importlib.import_module("core.utils.my_cycle_sample")
    out, warp = {}, {}
    for i, (H, W) in enumerate(fc.SIZES):
        tag = f"{H}x{W}"
        B = fc.FIXTURE_BATCH[(H, W)]
        flow = fc.make_flow(B, H, W, seed=10 + i)
        ft = torch.from_numpy(flow)
        assert np.array_equal(flow.astype(np.float16).astype(np.float32), flow)
        out[f"flow_{tag}"] = flow.astype(np.float16)
        out[f"omni_{tag}"] = np.stack([fv.omniflow_to_image(ft[b].clone()) for b in range(B)])
        out[f"plane_{tag}"] = np.stack([fv.flow_to_image(flow[b].transpose(1, 2, 0).copy()) for b in range(B)])
        sd = sph.calculate_veclen_spherical(ft.clone()).numpy()
        out[f"sd_{tag}"] = sd
        out[f"clip_{tag}"] = np.stack([np.sort(sd[b], axis=None)[int(0.95 * H * W)] for b in range(B)]).astype(np.float32)
        img = fc.make_image(1, fc.FIXTURE_WARP[(H, W)], H, W, seed=10 + i)            # the first image of the batch only
        warp[f"image_{tag}"] = img.astype(np.uint8)
        warp[f"warp_{tag}"] = cyc.my_cycle_warp(torch.from_numpy(img).clone(), ft[:1].clone()).numpy()
    f0 = torch.from_numpy(out["flow_64x128"][0].astype(np.float32))
    out["omni_bgr_64x128"] = fv.omniflow_to_image(f0.clone(), convert_to_bgr=True)[None]
    # hand cases, checked on the reference: zero flow -> every byte 255; an integer pan by k -> roll(x, -k)
    z = fv.omniflow_to_image(torch.zeros(2, 16, 32))
    assert (z == 255).all()
    x = torch.from_numpy(fc.make_image(1, 3, 16, 32, seed=3))
    pan = torch.zeros(1, 2, 16, 32)
    pan[:, 0] = 5.0
    assert torch.equal(cyc.my_cycle_warp(x.clone(), pan), torch.roll(x, -5, dims=3))
    total = 0
    for name, arrays in (("flow_viz.npz", out), ("flow_viz_warp.npz", warp)):
        path = os.path.join(_HERE, "golden", name)
        np.savez_compressed(path, **arrays)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)            # no committed file above 1 MiB
        total += os.path.getsize(path)
    assert total <= 1500000, total


if __name__ == "__main__":
    main()
