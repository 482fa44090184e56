"""Child process of tests/test_hip_dma_tall_tiles.py:
   python tests/run_tall_tile_case.py OUT.pt      (PRIORFLOW_DMA_TALL picks the planner's rule; it is read once per process)
Runs the 3x3 all-DMA launches of CASES on seeded buffers (conv_launches.build_case: the same bits in every process), checks each
against float64 with the sentinels (conv_launches.reference / check_case) and saves every output buffer, the plan
(pf_conv2d_tile, pf_conv2d_roles) and the failures."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FAKE = 0x1000

# name: (B, H, W, cin, cout, groups, co_groups, precision, epilogue, outputs, off_out, plan with the rule, plan without)
#   outputs: "f32" rows only, "twin" twin / f16 map only, "both"; the planner's codes: tile 3 / 4 = NT 1 / 2, roles 17 / 18 = the
#   128- / 256-pixel tile.  The smallest shapes at which the 256-pixel tiles can go wrong:
CASES = {
    # two full 8-row tiles; ONE chunk: the pipeline's first and last step coincide
    "full_tiles_one_chunk": (1, 16, 32, 32, 128, 2, 0, 1, 1, "both", 0, (3, 18), (3, 17)),
    # partial last row tile (12 rows), partial column tile (40 columns), the next image inside the halo (B = 2); odd chunk count;
    # partial last 32-channel tile; twin only at a channel offset
    "ragged_cout126_twin_at_128": (2, 12, 40, 96, 126, 2, 0, 1, 1, "twin", 128, (3, 18), (3, 17)),
    # padded last chunk (272 = 8.5 chunks), one chain of two (co_groups 1), LINEAR
    "ragged_cin272": (2, 12, 40, 272, 128, 1, 1, 1, 0, "f32", 0, (3, 18), (3, 17)),
    # Cout 192 at the product's geometry: 96 items of 256 px x 64 instead of 128 items of 128 px x 128 (half of them half padding)
    "cout192_product_map": (1, 64, 128, 32, 192, 1, 1, 1, 1, "both", 0, (4, 18), (4, 17)),
    # the flow chain's launch: three groups of 64 channels
    "three_groups_cout64": (1, 16, 32, 96, 64, 3, 0, 1, 1, "f32", 32, (3, 18), (3, 17)),
    # B = 4, 32 x 64, Cout 128 in three groups: 384 items of 128 px x 64 before.  The rule counts rounds of the chip, so it takes
    # 192 items of 256 px x 64 (one round at 12.9 KB) rather than 384 of 256 px x 32 (two at 8.9 KB) ...
    "b4_cout128_three_groups": (4, 32, 64, 96, 128, 3, 0, 1, 1, "both", 0, (4, 18), (3, 17)),
    # ... and the 256 px x 32 tile's walk THROUGH item boundaries (384 items on at most 256 workgroups, odd chunk count: the
    # halo buffer's parity moves from item to item) runs where a 64-channel tile would be half padding: Cout 32
    "b4_cout32_384_items": (4, 64, 128, 96, 32, 3, 0, 1, 1, "both", 0, (3, 18), (3, 17)),
    # the f16 forms of the new instantiation (64-channel chunks): ragged, and through item boundaries with three chunks
    "f16_ragged": (2, 12, 40, 128, 126, 2, 0, 2, 1, "both", 0, (3, 18), (3, 17)),
    "f16_b4_cout32_384_items": (4, 64, 128, 192, 32, 3, 0, 2, 1, "twin", 0, (3, 18), (3, 17)),
}


def launch_of(lib, name):
    """The conv_launches.Launch of a case: descriptors with placeholder pointers, as the planners and build_case read them."""
    import conv_launches as cl
    from prior_flow_amd import _lib
    B, H, W, cin, cout, ng, co, prec, epi, outputs, off_out, _, _ = CASES[name]
    cpc = 64 if prec == 2 else 32
    width = off_out + (cout + cpc - 1) // cpc * cpc
    descs = []
    for _ in range(ng):
        d = _lib.ConvDesc()
        d.in0_split, d.lds0, d.c0 = FAKE, (cin + cpc - 1) // cpc, cin
        d.zeros, d.zeros_bytes = FAKE, 4096
        d.weight = d.bias = FAKE
        d.cout, d.off_out = cout, off_out
        if outputs in ("f32", "both"):
            d.out, d.ld_out = FAKE, width + 8
        if outputs in ("twin", "both"):
            d.out_split, d.lds_out = FAKE, width // cpc
        d.kh = d.kw = 3
        d.epilogue, d.scale, d.precision, d.stride, d.co_groups = epi, 1.0, prec, 1, co
        descs.append(d)
    return cl.Launch(cl.signature(lib, descs, B, H, W), B, H, W, [cl._layout(d) for d in descs], name)


def main(path):
    import torch

    import conv_launches as cl
    from prior_flow_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    res = {}
    for idx, name in enumerate(CASES):
        ln = launch_of(lib, name)
        case = cl.build_case(lib, ln, ln.B, ln.H, ln.W, dev, seed=300 + idx)
        plan = cl.plan(lib, case.descs, ln.B, ln.H, ln.W)
        cl.run_case(lib, case)
        fails, worst = cl.check_case(case, cl.reference(case))
        outs = {f"{gi}.{k}": g["T"][k].cpu() for gi, g in enumerate(case.groups) for k in ("out", "out_split") if k in g["T"]}
        res[name] = {"plan": plan, "fails": fails, "worst": worst, "outs": outs}
        print(f"{name}: plan {plan}  worst |err| / bound per element {worst['elem']:.3g}, aggregate {worst['agg']:.3g}  {fails}", flush=True)
        del case
    torch.save(res, path)


if __name__ == "__main__":
    main(sys.argv[1])
