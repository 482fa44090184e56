// pf_conv2d: the launch plan (validation, tile, kernel instantiation, roles, statistics blocks) and its dispatch, host side.
// The kernels live in pf_conv_mfma.hip (generic, halo and role-specialised kernels on fp32 activations), pf_enc_conv.hip
// (weights-stationary kernel) and pf_conv_dma.hip (all-DMA kernel on pre-split activations).
#include <stdlib.h>
#include "pf_conv_priv.h"

using namespace pfconv;

// validation of the descriptors + geometry (conv_plan)
static int conv_prepare(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8,
                        ConvGroups& grp, ConvGeom& g, int& max_cout) {   // H8, W8: OUTPUT map size
    if (!descs || ngroups < 1 || ngroups > MAX_GROUPS) return PF_ERR_BAD_ARG;
    if (B <= 0 || H8 <= 0 || W8 <= 0) return PF_ERR_BAD_SHAPE;
    max_cout = 0;
    const pf_conv_desc& f = descs[0];
    for (int i = 0; i < ngroups; ++i) {
        const pf_conv_desc& d = descs[i];
        if ((!d.in0 && !d.in0_split) || !d.weight || !d.bias || (!d.out && !d.out_split)) return PF_ERR_BAD_ARG;
        if (d.c0 <= 0 || d.c1 < 0 || (d.c1 > 0 && !d.in1 && !d.in1_split)) return PF_ERR_BAD_ARG;
        // split twins (include/priorflow_hip.h): bf16x3 arithmetic, chunk-aligned slices that fit their rows; f16 maps (PF_PREC_F16):
        // the same with 64-channel chunks, and the operands exist in that form only
        const bool f16 = d.precision == PF_PREC_F16;
        const int cpc = f16 ? 64 : 32, cm = cpc - 1;         // channels per 128-byte chunk of an operand row
        if ((d.in0_split || d.in1_split || d.out_split || d.aux_split) && d.precision != PF_PREC_BF16X3 && !f16) return PF_ERR_BAD_ARG;
        if (f16 && (!d.in0_split || (d.c1 > 0 && !d.in1_split))) return PF_ERR_BAD_ARG;
        if (d.in0_split && ((d.off0 & cm) || d.lds0 * cpc < d.off0 + d.c0)) return PF_ERR_BAD_SHAPE;
        if (d.in1_split && d.c1 > 0 && ((d.off1 & cm) || (d.c0 & cm) || d.lds1 * cpc < d.off1 + d.c1)) return PF_ERR_BAD_SHAPE;
        // The all-DMA kernel copies whole chunks: a slice that ends inside a chunk must end at the END OF THE ROW, where
        // the operand row's columns past the logical width are zero by contract (anywhere else it would multiply a neighbour's live
        // columns -- possibly Inf / NaN -- by the zero-padded weights)
        if (d.in0_split && d.c1 == 0 && (d.c0 & cm) && d.off0 + ((d.c0 + cm) & ~cm) != d.lds0 * cpc) return PF_ERR_BAD_SHAPE;
        if (d.in1_split && d.c1 > 0 && (d.c1 & cm) && d.off1 + ((d.c1 + cm) & ~cm) != d.lds1 * cpc) return PF_ERR_BAD_SHAPE;
        if (d.out_split && ((d.off_out & 31) || d.lds_out <= 0)) return PF_ERR_BAD_SHAPE;
        if (d.aux_split && d.lds_aux * cpc < 128) return PF_ERR_BAD_SHAPE;
        if (d.pre && (d.off_pre < 0 || d.off_pre + d.cout > d.ld_pre)) return PF_ERR_BAD_SHAPE;
        if ((d.in0_split != nullptr) != (f.in0_split != nullptr) || (d.c1 > 0 && (d.in1_split != nullptr) != (d.in0_split != nullptr)))
            return PF_ERR_BAD_ARG;              // every group and both segments agree on the operand form
        // same geometry in every group: one kernel, one K loop
        if (d.kh != f.kh || d.kw != f.kw || d.c0 + d.c1 != f.c0 + f.c1) return PF_ERR_BAD_SHAPE;
        // odd k: window [-k/2, k/2]; even k: [-k/2, k/2 - 1] (the space-to-depth form of the 7x7/2 stem)
        if (d.kh < 1 || d.kw < 1 || d.kh > 7 || d.kw > 7 || d.cout <= 0) return PF_ERR_BAD_SHAPE;
        // 16-byte loads: every channel offset / stride must be a multiple of 4 floats
        if ((d.off0 | d.c0 | d.c1) & 3) return PF_ERR_BAD_SHAPE;
        if (d.in0 && (d.ld0 & 3)) return PF_ERR_BAD_SHAPE;
        if (d.c1 > 0 && ((d.off1 & 3) || (d.in1 && (d.ld1 & 3)) || (d.c0 % KC) != 0)) return PF_ERR_BAD_SHAPE;
        if (d.off0 < 0 || (d.in0 && d.off0 + d.c0 > d.ld0) || (d.c1 > 0 && (d.off1 < 0 || (d.in1 && d.off1 + d.c1 > d.ld1))))
            return PF_ERR_BAD_ARG;
        if (d.epilogue < PF_EPI_LINEAR || d.epilogue > PF_EPI_ADD) return PF_ERR_BAD_ARG;
        if ((d.epilogue == PF_EPI_RELU_RES || d.epilogue == PF_EPI_MASK || d.epilogue == PF_EPI_ADD) && (!d.h || d.ld_h < d.cout)) return PF_ERR_BAD_ARG;
        if (d.save_gates && d.aux_out && ((d.epilogue == PF_EPI_GRU_ZR && d.ld_aux < 256) || (d.epilogue == PF_EPI_GRU_Q && d.ld_aux < 128)))
            return PF_ERR_BAD_ARG;
        if (d.stride != f.stride || (d.stride != 1 && d.stride != 2)) return PF_ERR_BAD_SHAPE;
        if ((d.in_scale == nullptr) != (d.in_shift == nullptr)) return PF_ERR_BAD_ARG;
        if (d.epilogue == PF_EPI_TANH_RELU && (d.cout != 256 || (!d.aux_out && !d.aux_split) || (d.aux_out && d.ld_aux < 128))) return PF_ERR_BAD_ARG;
        if (d.precision != f.precision || (d.precision != PF_PREC_F32 && d.precision != PF_PREC_BF16X3 && !f16))
            return PF_ERR_BAD_ARG;
        const int out_w = (d.epilogue == PF_EPI_GRU_ZR || d.epilogue == PF_EPI_TANH_RELU) ? 128 : d.cout;
        if (d.off_out < 0 || (d.out && d.off_out + out_w > d.ld_out) || (d.out_split && d.off_out + out_w > d.lds_out * cpc))
            return PF_ERR_BAD_ARG;
        if (d.epilogue == PF_EPI_GRU_ZR && (d.cout != 256 || !d.h || (!d.aux_out && !d.aux_split) || (d.aux_out && d.ld_aux < 128) || d.ld_h < 128))
            return PF_ERR_BAD_ARG;
        if (d.epilogue == PF_EPI_GRU_Q && (d.cout != 128 || !d.h || !d.z || d.ld_z < 128 || d.ld_h < 128))
            return PF_ERR_BAD_ARG;
        grp.d[i] = d;
        if (d.cout > max_cout) max_cout = d.cout;
    }
    for (int i = ngroups; i < MAX_GROUPS; ++i) grp.d[i] = descs[0];
    g.H = H8; g.W = W8; g.N = H8 * W8; g.M = B * H8 * W8;
    g.kh = f.kh; g.kw = f.kw; g.taps = f.kh * f.kw;
    const int kc = f.precision == PF_PREC_F16 ? 64 : KC;     // channels per K-step of the kernel (F16: all-DMA kernel only)
    g.cin_pad = (f.c0 + f.c1 + kc - 1) / kc * kc;
    g.nchunks = g.cin_pad / kc;
    g.stride = f.stride; g.Hin = H8 * f.stride; g.Win = W8 * f.stride; g.Nin = g.Hin * g.Win;
    if (f.co_groups < 0 || f.co_groups > MAX_GROUPS) return PF_ERR_BAD_ARG;
    return PF_OK;
}

// Tile choice: the packed weights are zero-padded to a multiple of 128 output channels, so any
// BN in {32,64,128} is legal.  Small problems (one 512x1024 pair = 8192 pixels per branch) need
// the smaller tile to put >= 1 workgroup on each of the 256 CUs.
// 0: 128x32 (WM4 WN1 NT1)   1: 64x64 (WM2 WN2 NT1)   2: 64x128 (WM2 WN2 NT2)   7: 128x96 (WM4 WN1 NT3)
// 3: halo kernel 128x64     4: halo kernel 128x128   (bf16x3; any map size: edge tiles may be partial)
// 5: halo kernel 256x64 (8-row tile, Cout <= 64, 3x3 / 4x4, enough pixels to fill the chip)   8: halo kernel 256x96 (8-row tile, 3x3)
// `ngroups` here and in conv_dma_choice is the number of groups the chip sees at once: the launch's own plus pf_conv_desc.co_groups.
static int conv_tile(const ConvGeom& g, int ngroups, int max_cout, int precision) {
    const bool halo_shape = (g.kh == 3 && g.kw == 3) || (g.kh == 1 && g.kw == 5) || (g.kh == 5 && g.kw == 1) ||
                            (g.kh == 4 && g.kw == 4) || (g.kh == 1 && g.kw == 1);
    if ((precision == PF_PREC_BF16X3 || precision == PF_PREC_F16) && halo_shape && g.stride == 1) {
        const long B = g.M / g.N;
        const long tiles4 = B * ((g.H + 3) / 4) * ((g.W + 31) / 32), tiles8 = B * ((g.H + 7) / 8) * ((g.W + 31) / 32);
        const long wgs128 = tiles4 * ngroups * ((max_cout + 127) / 128);
        if (max_cout <= 64 && g.kh == g.kw && g.kh > 1 && tiles8 * ngroups >= 512) return 5;
        // 8: 256 px x 96 channels (TH 8, NT 3; round 6) -- the 3x3 96 -> 96 convolutions of the encoders' layer 2: no padding channels
        if (max_cout > 64 && max_cout <= 96 && g.kh == 3 && g.kw == 3 && tiles8 * ngroups >= 256) return 8;
        return (max_cout > 64 && wgs128 >= 256) ? 4 : 3;
    }
    const long m_tiles64 = ((long)g.M + 63) / 64 * ngroups;
    if (max_cout <= 32) return 0;
    // 7: 128 px x 96 channels (WM4 WN1 NT3; round 6) -- the encoders' layer 2 has 96 output channels, which the 128-channel tile
    // covers with a quarter of its weight loads and MFMAs on padding
    if (max_cout > 64 && max_cout <= 96 && ((long)g.M + 127) / 128 * ngroups >= 256) return 7;
    if (max_cout <= 64 || m_tiles64 * ((max_cout + 127) / 128) < 512) return 1;
    return 2;
}

// The shapes and options of the all-DMA and the role-specialised kernels: 3x3, 1x5, 5x1 stride 1, no input affine, no fused statistics
static bool roles_apply(const ConvGroups& grp, int ngroups, const ConvGeom& g) {
    if (!((g.kh == 3 && g.kw == 3) || (g.kh == 1 && g.kw == 5) || (g.kh == 5 && g.kw == 1)) || g.stride != 1) return false;
    for (int i = 0; i < ngroups; ++i)
        if (grp.d[i].stats_out != nullptr || grp.d[i].in_scale != nullptr) return false;
    return true;
}

// What one tile of pf_conv_dma_kernel<NT, ., ., WN> costs a launch -- the two numbers its tile choice is made of:
//   items       work items of the launch: pixel tiles (TH = 8 / WN rows x 32 columns; a ragged map's partial tiles count as whole
//               ones -- a 12-row map has two 8-row tiles, one of them half empty) x channel tiles of BN = 32 * NT * WN x groups
//   step_bytes  bytes a workgroup stages L2 -> LDS per K-step (one tap of one 128-byte operand chunk): a weight tile of BN rows
//               of 128 bytes, plus the chunk's halo -- (TH + kh - 1) x (32 + kw - 1) rows, rounded up to the 32-row pieces the
//               loaders issue -- spread over its kh * kw taps.  3x3: <1,2> 11.1 KB, <1,1> 8.9, <2,2> 19.1, <2,1> 12.9
// MFMA-busy is 0.09-0.15 on these launches, so a workgroup's time is taken as (items it walks) x (K-steps, the same on every
// tile) x step_bytes.  Measured, that overstates what the bytes buy at NT = 1 (-20 % of the bytes: -5 % of the launch; DESIGN.md
// section 6 has the table), but the order of the candidates it gives is the measured one.
struct DmaTileCost { long items, step_bytes; };
static DmaTileCost dma_tile_cost(const ConvGeom& g, int ngroups, int max_cout, int nt, int wn) {
    const int th = 8 / wn, bn = 32 * nt * wn;
    const long tiles = (long)(g.M / g.N) * ((g.H + th - 1) / th) * ((g.W + 31) / 32);
    const long halo_rows = ((long)(th + g.kh - 1) * (32 + g.kw - 1) + 31) / 32 * 32;
    return {tiles * ((max_cout + bn - 1) / bn) * ngroups, (long)bn * 128 + halo_rows * 128 / g.taps};
}

// The tile of a 3x3 all-DMA launch, as NT * 4 + WN: the one whose busiest workgroup stages the fewest bytes.  The launch and
// its `co` co-launched neighbours share the chip's 256 CUs evenly, so the busiest CU of the launch's share walks
// rounds = ceil(items * (ngroups + co) / (ngroups * 256)) items, and per K-step of the convolution it stages rounds * step_bytes.
// Ties go to the fewer bytes staged in total (items * step_bytes: L2 traffic and power), then to `prior`, the tile the
// work-item thresholds of conv_tile / conv_dma_choice give.  At one pair this means --
//   * the 256-pixel tile of the same NT wherever it has no more items than the 128-pixel one: 8.9 KB per step instead of 11.1
//     (Cout 128 / 126 in two chains, the three 64-channel convs of the flow chain), 12.9 instead of 19.1 (NT = 2);
//   * <2,3,3,1> for Cout 192: 96 items of 12.9 KB, nothing padded, instead of 128 items of 19.1 KB a quarter of whose weight rows
//     are zero padding -- it beats the two rounds of <1,3,3,1> (192 items, 2 x 8.9 KB) wherever its items fit the share in one;
// and at batch it keeps <2,3,3,1> (per output its 12.9 KB / 64 channels stay below 8.9 KB / 32).
// A one-group launch that has the chip to itself (co_groups 0) keeps `prior`: every measurement behind the model was
// taken with two chains or several groups sharing the chip; the encoders' and the last iteration's launches stay as they were.
// 1x5 / 5x1 keep conv_dma_choice's rules: the same arithmetic gives the 8-row tile of NT = 1 only -7 % (1x5: 11.2
// against 12.0 KB) and -6 % (5x1: 13.6 against 14.4 KB) there, too little to tell from noise in the forward.
// PRIORFLOW_DMA_TALL=0 (A/B knob, read once per process): `prior`, and the tile / roles report that went with it, everywhere.
static bool dma_tall_rules() {
    static const bool on = [] { const char* e = getenv("PRIORFLOW_DMA_TALL"); return !e || atoi(e) != 0; }();
    return on;
}
static int conv_dma_tile_3x3(const ConvGeom& g, int ngroups, int co, int max_cout, int prior) {
    constexpr long CUS = 256;
    const long chip = ngroups + co;
    if (chip < 2) return prior;
    int best = -1;
    long best_crit = 0, best_total = 0;
    for (const int cand : {prior, 1 * 4 + 1, 2 * 4 + 1, 1 * 4 + 2, 2 * 4 + 2}) {        // prior first: it wins every tie
        if (best >= 0 && (cand >> 2) == 2 && max_cout <= 32 * (cand & 3)) continue;       // NT = 2 on one 32 * WN channel block: padding only
        const DmaTileCost c = dma_tile_cost(g, ngroups, max_cout, cand >> 2, cand & 3);
        const long rounds = (c.items * chip + ngroups * CUS - 1) / (ngroups * CUS);
        const long crit = rounds * c.step_bytes, total = c.items * c.step_bytes;
        if (best < 0 || crit < best_crit || (crit == best_crit && total < best_total)) { best = cand; best_crit = crit; best_total = total; }
    }
    return best;
}

// Pre-split operands (pf_conv_desc.in0_split): which tile the all-DMA kernel takes -- 0: not applicable (fp32 operands,
// a shape / option it does not implement), else the pf_conv2d_roles code (1: 128-px tile, 2: 256 px x 64 channels; a 3x3
// launch on tile 3 / 4 then goes through conv_dma_tile_3x3, which may move it to another tile of the same kernel).
// (The engine's PRIORFLOW_PRESPLIT=0 is the A/B against the register-staged kernels: it hands over fp32 operands.)
// PF_PREC_F16 exists on this kernel only: a launch it does not take is an error for the caller (conv_plan), never a fallback.
static int conv_dma_choice(const ConvGroups& grp, int ngroups, const ConvGeom& g, int max_cout, int tile_id) {
    if (!grp.d[0].in0_split || tile_id < 3 || tile_id == 7 || !roles_apply(grp, ngroups, g)) return 0;
    if (tile_id == 5) return 2;            // Cout <= 64 on a big map (3x3 by conv_tile's rule): the 256 px x 64 channel tile
    const long wgs256 = (long)(g.M / g.N) * ((g.H + 7) / 8) * ((g.W + 31) / 32) * (ngroups + grp.d[0].co_groups) * ((max_cout + 63) / 64);
    // round 4: the 256 px x 64 channel tile for the 1x5 / 5x1 convolutions with Cout > 128 (the GRU's fused z|r) too: half the
    // weight bytes staged per output, twice the halo; +0.2 % at B = 1, +0.6 % at batch 32 (profiles/r4_ab_gru_tile.txt)
    if (g.kh != 3 && max_cout > 128 && wgs256 >= 256) return 2;
    return (g.kh == 3 && max_cout > 64 && wgs256 >= 256) ? 2 : 1;
}

// Which form of the halo kernel a TH = 4 launch takes: 0 the symmetric pf_conv_halo_kernel, 1 pf_conv_ws_kernel with the
// call's own 128-px tile (WN = 2), 2 pf_conv_ws_kernel with the 256 px x 64 channel tile (WN = 1; only where that still
// gives every CU a workgroup).  PRIORFLOW_CONV_WS (A/B knob): 0 / 1 cap the choice, default 2.
static int conv_ws_choice(const ConvGroups& grp, int ngroups, const ConvGeom& g, int max_cout) {
    static const int ws = [] { const char* e = getenv("PRIORFLOW_CONV_WS"); return e ? atoi(e) : 2; }();
    if (ws <= 0 || !roles_apply(grp, ngroups, g)) return 0;
    const long wgs256 = (long)(g.M / g.N) * ((g.H + 7) / 8) * ((g.W + 31) / 32) * ngroups * ((max_cout + 63) / 64);
    // (measured: the 256-px tile wins for the 3x3 convs, -2 % at B=1; for 1x5 / 5x1 its taller halo costs more than the weights save)
    if (ws >= 3 && g.kh == 3 && wgs256 >= 256) return 2;       // A/B: the 256 px x 64 channel roles kernel for Cout <= 64 as well
    return (ws >= 2 && g.kh == 3 && max_cout > 64 && wgs256 >= 256) ? 2 : 1;
}

// The plan of one launch: PF_OK, or the PF_ERR_* code with which pf_conv2d refuses the descriptors.  Every decision about a
// pf_conv2d launch is made here, once; pf_conv2d runs p.launch and the three queries read one field each.
static int conv_plan(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8, ConvPlan& p) {
    if (const int rc = conv_prepare(descs, ngroups, B, H8, W8, p.grp, p.g, p.max_cout)) return rc;
    const ConvGroups& grp = p.grp;
    const ConvGeom& g = p.g;
    p.ngroups = ngroups;
    p.tile = conv_tile(g, ngroups + descs[0].co_groups, p.max_cout, descs[0].precision);
    const int dma = conv_dma_choice(grp, ngroups, g, p.max_cout, p.tile);
    if (descs[0].precision == PF_PREC_F16 && !dma) return PF_ERR_BAD_SHAPE;     // f16 operands exist on the all-DMA kernel only
    const bool split = descs[0].precision == PF_PREC_BF16X3;
    const bool generic = p.tile < 3 || p.tile == 7;
    const int bm = (p.tile == 0 || p.tile == 7) ? 128 : 64;  // generic kernel: tiles of bm consecutive pixels, which must not straddle images
    for (int i = 0; i < ngroups; ++i) {     // the input affine is implemented by the halo kernel only; the fused statistics by the
        if (descs[i].in_scale && generic) return PF_ERR_BAD_SHAPE;          // halo kernel and (round 4) by the generic one when its
        if (descs[i].stats_out && descs[i].epilogue != PF_EPI_LINEAR) return PF_ERR_BAD_SHAPE;     // M tiles do not straddle images
        if (descs[i].stats_out && generic && (!split || g.N % bm != 0)) return PF_ERR_BAD_SHAPE;
    }
    // tile 5 (Cout <= 64 on a big map) with 64 input channels: the weights-stationary kernel, bit-identical to the halo kernel
    const bool enc64 = (p.tile == 5 || p.tile == 3) && pf_enc_conv64_applies(grp, ngroups, g, p.max_cout);
    // statistics partials per image of the launch with stats_out (which never takes the all-DMA kernel): the weights-stationary
    // kernel's per (segment, row phase, strip), the halo kernels' per pixel tile, the generic kernel's per bm pixels
    const int th = (p.tile == 5 || p.tile == 8) ? 8 : 4;
    p.stats_blocks = enc64 ? pf_enc_conv64_stats_blocks(g)
                   : generic ? ((split && g.N % bm == 0) ? g.N / bm : 0) : ((g.H + th - 1) / th) * ((g.W + 31) / 32);
    p.affine = false;
    if (dma) {                              // pre-split operands: the all-DMA kernel, which reads its zero padding from memory
        for (int i = 0; i < ngroups; ++i)
            if (!descs[i].zeros || descs[i].zeros_bytes < 128 * (descs[i].lds0 > descs[i].lds1 ? descs[i].lds0 : descs[i].lds1)) return PF_ERR_BAD_ARG;
        int nt = (dma == 2 || p.tile == 4) ? 2 : 1, wn = dma == 2 ? 1 : 2;
        if (g.kh == 3 && (p.tile == 3 || p.tile == 4) && dma_tall_rules()) {
            // tiles 5 and 8 are <2,3,3,1> by conv_tile's own rules (big maps) and stay.  Here the reported tile follows the
            // kernel: 3 / 4 = NT 1 / 2, roles 16 + 1 / 16 + 2 = the 128- / 256-pixel tile.  (Without this rule, and for the
            // 1x5 / 5x1 launches still, the report has tile 3 with 16 + 2 where <2,.,.,1> runs on a map with wgs128 < 256 <= wgs256.)
            const int t = conv_dma_tile_3x3(g, ngroups, descs[0].co_groups, p.max_cout, nt * 4 + wn);
            nt = t >> 2; wn = t & 3;
            p.tile = nt == 1 ? 3 : 4;
        }
        p.roles = 16 + (wn == 1 ? 2 : 1);
        p.launch = wn == 1 ? (nt == 2 ? pf_conv_dma_launch<2, 1> : pf_conv_dma_launch<1, 1>)
                           : (nt == 2 ? pf_conv_dma_launch<2, 2> : pf_conv_dma_launch<1, 2>);
        return PF_OK;
    }
    for (int i = 0; i < ngroups; ++i) {
        if (!descs[i].in0 || (descs[i].c1 > 0 && !descs[i].in1)) return PF_ERR_BAD_ARG;   // fp32 operands needed from here on
        if (descs[i].pre) return PF_ERR_BAD_SHAPE;                                          // accumulator start values: all-DMA kernel only
    }
    p.roles = 0;
    if (enc64) { p.tile = 6; p.launch = pf_enc_conv64_launch; return PF_OK; }
    if (!generic) {                         // every group agrees on having an input affine (one instantiation per launch)
        p.affine = descs[0].in_scale != nullptr;
        for (int i = 1; i < ngroups; ++i)
            if ((descs[i].in_scale != nullptr) != p.affine) return PF_ERR_BAD_ARG;
        if (p.affine && (g.kh != 3 || g.kw != 3)) return PF_ERR_BAD_SHAPE;   // only the encoders' 3x3 convs use it
    }
    if (p.tile == 3 || p.tile == 4) p.roles = conv_ws_choice(grp, ngroups, g, p.max_cout);
    switch (p.tile) {
        case 0: p.launch = pf_conv_generic_launch<4, 1, 1>; break;
        case 1: p.launch = pf_conv_generic_launch<2, 2, 1>; break;
        case 2: p.launch = pf_conv_generic_launch<2, 2, 2>; break;
        case 7: p.launch = pf_conv_generic_launch<4, 1, 3>; break;
        case 3: p.launch = p.roles == 2 ? pf_conv_ws_launch<2, 1> : p.roles == 1 ? pf_conv_ws_launch<1, 2> : pf_conv_halo_launch<1, 4>; break;
        case 4: p.launch = p.roles == 2 ? pf_conv_ws_launch<2, 1> : p.roles == 1 ? pf_conv_ws_launch<2, 2> : pf_conv_halo_launch<2, 4>; break;
        case 5: p.launch = pf_conv_halo_launch<2, 8>; break;
        default: p.launch = pf_conv_halo_launch<3, 8>; break;     // 8
    }
    return PF_OK;
}

extern "C" int pf_conv2d_tile(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8) {
    ConvPlan p;
    const int rc = conv_plan(descs, ngroups, B, H8, W8, p);
    return rc != PF_OK ? rc : p.tile;
}

extern "C" int pf_conv2d_stats_blocks(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8) {
    ConvPlan p;
    const int rc = conv_plan(descs, ngroups, B, H8, W8, p);
    return rc != PF_OK ? rc : p.stats_blocks;
}

extern "C" int pf_conv2d_roles(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8) {
    ConvPlan p;
    const int rc = conv_plan(descs, ngroups, B, H8, W8, p);
    return rc != PF_OK ? rc : p.roles;
}

extern "C" int pf_conv2d(const pf_conv_desc* descs, int ngroups, int B, int H8, int W8, void* stream) {
    ConvPlan p;
    const int rc = conv_plan(descs, ngroups, B, H8, W8, p);
    return rc != PF_OK ? rc : p.launch(p, (hipStream_t)stream);
}
