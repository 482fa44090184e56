"""Driver for a kernel trace of the flow renderer: 30 x (render + warp with residual and mean) at 512x1024, B = 1 (DESIGN.md
section 13).  Run it under the profiler, in a run of its own, and keep the kernel summary:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o r9_flow_viz -- python profiles/trace_flow_viz.py
    -> OUT/r9_flow_viz_kernel_stats.csv, committed as profiles/r9_flow_viz_kernel_stats.csv
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from prior_flow_amd import synthetic_pair  # noqa: E402
from prior_flow_amd.flow_viz import FlowRenderer  # noqa: E402


def main():
    B, H, W = 1, 512, 1024
    im1, im2 = (t.cuda().contiguous() for t in synthetic_pair(B, H, W, seed=7))
    g = torch.Generator().manual_seed(5)
    flow = (4.0 * torch.randn(B, 2, H, W, generator=g)).cuda()
    r = FlowRenderer(B, H, W, "cuda")
    r.prepare_warp(3)
    for _ in range(30):
        r.render(flow)
        r.warp(im2, flow, image1=im1)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
