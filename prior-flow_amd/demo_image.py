"""``python -m prior_flow_amd.demo_image --img1 A.png --img2 B.png [--model CKPT] [--out flow_pr.png]``

The reference's ``demo_image.py``: the flow of one image pair (iters = 12, test mode), colour coded with ``omniflow_to_image``
and written as a PNG.  Images are read and written with PIL (RGB in, RGB out: the same file the reference's
``cv2.imwrite(cvtColor(RGB2BGR))`` writes).  Without ``--model`` the deterministic ``det_state_dict`` weights are used, which
exercises the pipeline but predicts nothing meaningful; the script says so.
"""
from __future__ import annotations

import argparse
from typing import Optional, Sequence

import numpy as np
import torch

from . import det_state_dict
from .flow_viz import omniflow_to_image
from .prior_raft import PriOr_RAFT, state_dict_shapes


def load_image(imfile: str, device="cuda") -> torch.Tensor:
    from PIL import Image
    img = np.array(Image.open(imfile).convert("RGB")).astype(np.uint8)
    return torch.from_numpy(img).permute(2, 0, 1).float()[None].to(device)


def build_model(args) -> PriOr_RAFT:
    model = PriOr_RAFT(args)
    if args.model:
        raw = torch.load(args.model, map_location="cpu")
        raw = {(k[7:] if k.startswith("module.") else k): v for k, v in raw.items()}       # DataParallel checkpoints
        model.load_state_dict(raw, strict=True)
    else:
        print("[demo_image] no --model given: using the deterministic det_state_dict weights (the flow is not a prediction)")
        model.load_state_dict(det_state_dict(state_dict_shapes()), strict=True)
    return model.cuda().eval()


def run(args, model: Optional[PriOr_RAFT] = None) -> torch.Tensor:
    """Flow of the pair -> colour image [H,W,3] uint8 (device tensor), also written to ``args.out``."""
    from PIL import Image
    model = build_model(args) if model is None else model
    image1, image2 = load_image(args.img1), load_image(args.img2)
    with torch.no_grad():
        flow_pr = model(image1, image2, iters=args.iters, test_mode=True)
    colored = omniflow_to_image(flow_pr[0])
    Image.fromarray(colored.cpu().numpy()).save(args.out)
    print(f"[demo_image] flow {tuple(flow_pr.shape)} -> {args.out}")
    return colored


def parse_args(argv: Optional[Sequence[str]] = None):
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--model", default=None, help="restore checkpoint (default: deterministic synthetic weights)")
    parser.add_argument("--img1", type=str, required=True, help="path of image1")
    parser.add_argument("--img2", type=str, required=True, help="path of image2")
    parser.add_argument("--out", type=str, default="./flow_pr.png", help="where the colour-coded flow is written")
    parser.add_argument("--iters", type=int, default=12)
    parser.add_argument("--mixed_precision", action="store_true", help="use mixed precision")
    parser.add_argument("--dropout", type=float, default=0.0)
    return parser.parse_args(argv)


if __name__ == "__main__":
    run(parse_args())
