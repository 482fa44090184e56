"""The launch rules of tests/launch_paths.py are those of the sources, and the cases built on them reach what they are there for
(DESIGN.md sections 25 and 26): every constant and rule is pinned to the text of csrc/pf_segments.hip, csrc/pf_tracker.hip and
csrc/pf_tracker.h, so a change in a launcher has to be noticed here; sc.DEVICE_PATHS and tc.DEVICE_PATHS reach their paths on cards
of 32, 64, 256 and 304 CUs; no shape of sc.SWEEP or tc.SHAPES reaches any of them on a whole MI355X.  The same for the LDS window
of pf_splat_acc_kernel (section 18) and for the grids with a fixed cap of the order statistic, the render (section 13) and the
augmentor (section 14): their rules do not depend on the CU count."""
import os
import re

import numpy as np

import augment_cases as ac
import flow_viz_cases as fc
import flow_viz_checks as ck
import launch_paths as lp
import segments_cases as sc
import splat_cases as spc
import splat_ref as sr
import tracker_cases as tc

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "prior-flow_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(text, kernel):
    """The text of one kernel: from its name to the next __global__ (or the end of the anonymous namespace)."""
    at = text.index(kernel + "(const ")
    ends = [e for e in (text.find("__global__", at), text.find("}  // namespace", at)) if e > 0]
    return text[at:min(ends)]


def test_constants_and_rules_are_those_of_the_sources():
    seg, trk, trk_h = _text("pf_segments.hip"), _text("pf_tracker.hip"), _text("pf_tracker.h")
    assert "constexpr int kFlat = 1024;" in seg and lp.K_FLAT == 1024
    assert "constexpr int kLdsObjects = 512;" in seg and lp.K_LDS_OBJECTS == 512
    assert "constexpr int kBlock = 256, kWaves = kBlock / 64;" in seg and lp.K_SCAN_BLOCK == 256
    assert "constexpr int kVote = 1024, kVoteWaves = kVote / 64;" in trk and (lp.K_VOTE, lp.K_VOTE_WAVES) == (1024, 16)
    assert re.search(r"^#define PF_TK_LDS_OBJECTS 64\b", trk_h, re.M) and lp.TK_LDS_OBJECTS == 64
    assert "PF_SEG_MAX_OBJECTS == 4096" in _text("pf_segments.h") and lp.SEG_MAX_OBJECTS == 4096
    assert "PF_TRK_MAX_OBJECTS == 256" in trk_h and lp.TRK_MAX_OBJECTS == 256
    # the grids: wanted, the cap, the smaller of the two; which kernel a table size takes
    assert "const long want = pf_sg_blocks((long)H * W, kFlat), cap = (2L * pf_sg_cus() + B - 1) / B;" in seg
    assert "const dim3 acc_grid((unsigned)(want < cap ? want : cap), (unsigned)B);" in seg
    assert "if (max_objects <= kLdsObjects)\n        hipLaunchKernelGGL(pf_seg_objects_accumulate<true>, acc_grid, dim3(kFlat)," in seg
    assert "const long items = (long)a.H * ((a.W + 63) / 64);" in trk
    assert "const long want = pf_tk_blocks(items, kVoteWaves), cap = (2L * pf_tk_cus() + a.B - 1) / a.B;" in trk
    assert "const dim3 grid((unsigned)(want < cap ? want : cap), (unsigned)a.B);" in trk
    assert "if (a.M <= PF_TK_LDS_OBJECTS)\n        hipLaunchKernelGGL(pf_trk_vote_kernel<true>, grid, dim3(kVote)," in trk
    for text in (seg, trk):
        assert "hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev)" in text
    # the loops that take the further trips, and the scan's rows per thread with its two clips
    acc, vote, scan = _body(seg, "pf_seg_objects_accumulate"), _body(trk, "pf_trk_vote_kernel"), _body(seg, "pf_seg_rank_scan")
    assert "for (long n = (long)blockIdx.x * kFlat + threadIdx.x; n < N; n += (long)gridDim.x * kFlat) {" in acc
    assert "for (long it = (long)blockIdx.x * kVoteWaves + wave; it < items; it += (long)gridDim.x * kVoteWaves) {" in vote
    assert "__launch_bounds__(kBlock) pf_seg_rank_scan" in seg and "hipLaunchKernelGGL(pf_seg_rank_scan, dim3((unsigned)B), dim3(kBlock)" in seg
    assert "const int per = (H + kBlock - 1) / kBlock;" in scan and "const long lo_l = (long)t * per;" in scan
    assert "const int lo = lo_l < H ? (int)lo_l : H, hi = lo_l + per < H ? (int)(lo_l + per) : H;" in scan
    assert "__launch_bounds__(kBlock) pf_trk_match_kernel" in trk and "constexpr int kBlock = 256;" in trk


def test_the_rules_themselves():
    assert lp.cap(1, 256) == 512 and lp.cap(2, 256) == 256 and lp.cap(3, 256) == 171 and lp.cap(512, 256) == 1 and lp.cap(513, 256) == 1
    assert lp.seg_accumulate_grid(2, 512, 1024, 256) == (512, 256) and lp.trips((512, 256)) == 2 and lp.trips((513, 256)) == 3
    assert lp.seg_accumulate_grid(1, 40, 1100, 256) == (43, 43) and lp.trk_vote_grid(1, 40, 1100, 256) == (45, 45)
    assert lp.trk_vote_grid(2, 512, 1024, 256) == (512, 256) and lp.trk_vote_grid(512, 24, 48, 256) == (2, 1)
    assert [lp.seg_scan_rows_per_thread(H) for H in (1, 256, 257, 512, 513, 600)] == [1, 1, 2, 2, 3, 3]
    for H in (1, 130, 256, 257, 512, 600, 1000):                     # the threads' spans tile the rows
        assert sum(lp.seg_scan_rows_of_thread(H, t) for t in range(lp.K_SCAN_BLOCK)) == H
        assert all(lp.seg_scan_rows_of_thread(H, t) < lp.seg_scan_rows_per_thread(H) for t in lp.clipped_threads(H))
        assert all(lp.seg_scan_rows_of_thread(H, t) == lp.seg_scan_rows_per_thread(H) for t in range(lp.clipped_threads(H).start))
    assert lp.clipped_threads(257) == range(128, 256) and lp.seg_scan_rows_of_thread(257, 128) == 1
    assert lp.clipped_threads(600) == range(200, 256) and lp.seg_scan_rows_of_thread(600, 200) == 0 and not len(lp.clipped_threads(512))


def test_the_device_path_cases_reach_their_paths_on_every_card():
    for cus in lp.CU_COUNTS:
        seg = {case: set().union(*(lp.seg_device_paths(*sc.device_case(case, cus), s[2], cus) for s in sc.DEVICE_SETTINGS))
               for case in sc.DEVICE_PATHS}
        both = {"accumulate_second_trip_lds", "accumulate_second_trip_global"}
        B, C, H, W = sc.device_case(sc.DEVICE_PATHS[0], cus)
        # one workgroup per image: a full trip of 1024 pixels and a ragged one of 128
        assert lp.seg_accumulate_grid(B, H, W, cus) == (2, 1) and H * W - lp.K_FLAT == 128
        assert both <= seg[sc.DEVICE_PATHS[0]] and both <= seg[(2, 3, 512, 1024)], cus
        assert lp.seg_accumulate_grid(2, 512, 1024, cus) == (512, cus)
        assert all({"table_512", "table_4096"} <= reached for reached in seg.values())
        assert {"scan_two_rows_per_thread"} <= seg[(2, 3, 512, 1024)] and "scan_clipped_threads" not in seg[(2, 3, 512, 1024)]
        for case, per in (((1, 1, 257, 66), 2), ((1, 0, 600, 8), 3)):
            assert {"scan_two_rows_per_thread", "scan_clipped_threads"} <= seg[case] and lp.seg_scan_rows_per_thread(case[2]) == per
        for case in tc.DEVICE_PATHS:
            B, H, W = tc.device_case(case, cus)
            reached = set().union(*(lp.trk_device_paths(B, H, W, s[0], cus) for s in tc.DEVICE_SETTINGS))
            assert {"vote_second_trip_lds", "vote_second_trip_global", "table_256"} <= reached, (case, cus)
        # 24 items for the 16 waves of the one workgroup: the waves from 8 find nothing in the second trip
        B, H, W = tc.device_case(tc.DEVICE_PATHS[0], cus)
        assert lp.trk_vote_grid(B, H, W, cus) == (2, 1) and H * ((W + 63) // 64) == lp.K_VOTE_WAVES + 8
    assert sc.DEVICE_PATHS[0][0] == tc.DEVICE_PATHS[0][0] == sc.TWO_PER_CU and sc.device_case(sc.DEVICE_PATHS[0])[0] == 512
    assert set(sc.FULL_TABLES) <= set(sc.DEVICE_SETTINGS) and tc.FULL_TABLE in tc.DEVICE_SETTINGS
    assert {s[2] for s in sc.FULL_TABLES} == {lp.K_LDS_OBJECTS, lp.SEG_MAX_OBJECTS} and tc.FULL_TABLE[0] == lp.TRK_MAX_OBJECTS


def test_no_shape_of_the_sweeps_reaches_them_on_a_whole_card():
    """The statement of the gap that the device-path cases close: on 256 CUs the sweeps take no second trip, hold one row per
    thread in the scan and stay below the tables' limits."""
    cus = 256
    for B, C, H, W in sc.SWEEP:
        for s in sc.SETTINGS:
            assert not lp.seg_device_paths(B, C, H, W, s[2], cus), (B, C, H, W, s)
        assert lp.trips(lp.seg_accumulate_grid(B, H, W, cus)) == 1 and lp.seg_scan_rows_per_thread(H) == 1
    assert max(lp.seg_accumulate_grid(B, H, W, cus)[1] for B, C, H, W in sc.SWEEP) == 43
    for B, H, W in tc.SHAPES:
        for M, _ in tc.SETTINGS:
            assert not lp.trk_device_paths(B, H, W, M, cus), (B, H, W, M)
    assert max(lp.trk_vote_grid(B, H, W, cus)[1] for B, H, W in tc.SHAPES) == 45
    assert max(s[2] for s in sc.SETTINGS) < lp.SEG_MAX_OBJECTS and lp.K_LDS_OBJECTS not in {s[2] for s in sc.SETTINGS}
    assert max(s[0] for s in tc.SETTINGS) < lp.TRK_MAX_OBJECTS


# ---- the LDS window of pf_splat_acc_kernel --------------------------------------------------------------------
def test_splat_window_constants_and_rules_are_those_of_the_sources():
    hip, h = _text("pf_splat.hip"), _text("pf_splat.h")
    assert "constexpr int kTileY = 8, kTileX = 64;" in hip and (lp.SPLAT_TILE_Y, lp.SPLAT_TILE_X) == (sr.TILE_Y, sr.TILE_X) == (8, 64)
    assert "constexpr int kMarginY = 4, kMarginX = 8;" in hip and (lp.SPLAT_MARGIN_Y, lp.SPLAT_MARGIN_X) == (4, 8)
    assert "constexpr int kWinY = kTileY + 2 * kMarginY, kWinX = kTileX + 2 * kMarginX, kCells = kWinY * kWinX;" in hip
    assert (lp.SPLAT_WIN_Y, lp.SPLAT_WIN_X) == (16, 80)
    assert "constexpr float kNear = 268435456.f;" in hip and lp.SPLAT_NEAR == 268435456.0 == 2.0 ** 28
    assert re.search(r"^#define PF_SPLAT_FAR 1073741824\.f", h, re.M) and lp.SPLAT_FAR == 1073741824.0 == sr.FAR
    acc = _body(hip, "pf_splat_acc_kernel")
    # the tile of a workgroup, its centre pixel, where that lands, whether a window is placed there, and the window's origin
    assert "const int tiles_x = (a.W + kTileX - 1) / kTileX;" in acc
    assert "const int ty0 = ((int)blockIdx.x / tiles_x) * kTileY, tx0 = ((int)blockIdx.x % tiles_x) * kTileX;" in acc
    assert "const int cy = min(ty0 + kTileY / 2, a.H - 1), cx = min(tx0 + kTileX / 2, a.W - 1);" in acc
    assert "const float* fl = q.flow + b * 2 * N + ((long)cy * a.W + cx);" in acc
    assert "const float qx = (float)cx + q.tau * fl[0], qy = (float)cy + q.tau * fl[N];" in acc
    assert "const bool ok = fabsf(qx) < kNear && fabsf(qy) < kNear;" in acc
    assert "const int ix = ok ? (int)floorf(qx) : cx, iy = ok ? (int)floorf(qy) : cy;" in acc
    assert "sink.oy = iy - (cy - ty0) - kMarginY;" in acc
    assert "int ox = (ix - (cx - tx0) - kMarginX) % a.W;" in acc and "sink.ox = ox < 0 ? ox + a.W : ox;" in acc
    assert "const int x = tx0 + (tid & 63);" in acc and "const int y = ty0 + (tid >> 6) + 4 * r;" in acc
    assert "dim3((unsigned)tiles, (unsigned)njobs, (unsigned)B)" in hip and "const long b = blockIdx.z" in acc
    # the window-or-direct choice of a tap, and the flush
    assert "int xr = xx - ox;\n        xr = xr < 0 ? xr + W : xr;\n        const int yr = yy - oy;" in hip
    assert "if ((unsigned)xr < (unsigned)kWinX && (unsigned)yr < (unsigned)kWinY)" in hip and "direct.add(plane, yy, xx, v);" in hip
    assert "sink.direct.add(plane, sink.oy + yr, (sink.ox + xr) % a.W, (long long)v);" in acc
    # the pixel and its taps (pf_splat.h), as splat_window_counts restates them
    assert "const float qx = (float)x + q.tau * fl[n], qy = (float)y + q.tau * fl[N + n];" in h
    assert "if (!(fabsf(qx) < PF_SPLAT_FAR && fabsf(qy) < PF_SPLAT_FAR)) return;" in h
    assert "int x0 = (int)x0f % W;" in h and "const int x1 = x0 + 1 == W ? 0 : x0 + 1;" in h
    assert "if (yy < 0 || yy >= H || !(bk > 0.f)) return;" in h


def test_splat_window_rules_themselves():
    """Hand cases at 8 x 128 (two tiles): zero flow keeps every tap inside; one far column, one far row, a straddling pixel."""
    H, W = 8, 128
    z = np.zeros((2, H, W), np.float32)
    c = lp.splat_window_counts(z, 1.0, H, W)
    assert c["tiles"] == 2 and c["window_taps"] == H * W and not (c["direct_x_taps"] or c["direct_y_taps"] or c["unplaced_tiles"])
    assert c["negative_origins"] == 1 and c["seam_tiles"] == 2          # origins -8 -> column 120 and 56: both + 80 > 128
    assert lp.splat_window_paths(z, 1.0, H, W) == {"seam_window", "negative_origin"}
    f = z.copy()
    f[0, 2, 3] = 72.0            # x = 3 lands on column 75: xr = 75 - (-8) = 83 >= 80
    f[1, 5, 70] = 8.0            # y = 5 lands on row 13: yr = 13 + 4 = 17 >= 16
    f[0, 1, 1] = -9.5            # x = 1 lands on -8.5: column -9 is outside (xr = 127), column -8 inside
    c = lp.splat_window_counts(f, 1.0, H, W)
    assert (c["direct_x_taps"], c["direct_y_taps"], c["split_pixels"]) == (2, 0, 1)      # row 13 is outside the map: dropped, not direct
    f[1, 5, 70] = -6.5           # rows -2 and -1: dropped as well
    f[1, 7, 70] = -12.5          # rows -6 (outside the map) and -5 ... also dropped
    f[1, 0, 100] = 7.0           # y = 0 -> row 7, inside
    assert lp.splat_window_counts(f, 1.0, H, W)["direct_y_taps"] == 0
    tall = np.zeros((2, 24, 64), np.float32)
    tall[1, 1, 5] = 12.0         # tile 0, y = 1 -> row 13: yr = 13 + 4 = 17
    tall[1, 9, 5] = -5.5         # tile 1 (rows 8..15), y = 9 -> rows 3 and 4: yr = -1 and 0
    c = lp.splat_window_counts(tall, 1.0, 24, 64)
    assert (c["direct_y_taps"], c["split_pixels"], c["direct_x_taps"]) == (2, 1, 0)
    # centres: (4, 32) of tile 0 at 8 x 128; NaN, inf and 2^28 are not placed, 2^28 - 64 is; a skipped pixel makes no tap
    for v, n in ((np.nan, 1), (np.inf, 1), (2.0 ** 28, 1), (2.0 ** 28 - 64, 0)):
        g = z.copy()
        g[0, 4, 32] = v
        assert lp.splat_window_counts(g, 1.0, H, W)["unplaced_tiles"] == n, v
    skip = np.zeros((1, H, W), np.uint8)
    skip[0, 2, 3] = 1
    assert lp.splat_window_counts(f, 1.0, H, W, skip)["direct_x_taps"] == 1
    assert lp.splat_window_paths(np.zeros((2, 2, 8, 72), np.float32), 1.0, 8, 72) >= {"narrow_map", "batched_columns", "clipped_centre"}
    assert "width_is_window" in lp.splat_window_paths(np.zeros((2, 8, 80), np.float32), 1.0, 8, 80)
    assert "three_columns" in lp.splat_window_paths(np.zeros((2, 8, 129), np.float32), 1.0, 8, 129)
    assert "narrow_map" not in lp.splat_window_paths(np.zeros((2, 8, 81), np.float32), 1.0, 8, 81)


SPLAT_NEW = {"centre_unplaced", "narrow_map", "width_is_window", "batched_columns", "three_columns", "clipped_centre"}


def test_the_splat_cases_reach_their_paths():
    """What every family, shape and setting of sc.DEVICE_PATHS reaches: the shape's paths at every case of the shape, an unplaced
    centre under every `centre_bad` case (and under `centre_far`), the torn and margin families the direct taps and the split
    pixels beside more than one tile column and more than one image."""
    reached = {case: spc.reached(case) for case in spc.DEVICE_PATHS}
    assert len(reached) == 5 * 4 * 3 and {c[1] for c in reached} == set(sr.DEVICE_SHAPES) and {c[2:] for c in reached} == set(sr.DEVICE_SETTINGS)
    by_shape = {(3, 20, 200): {"three_columns", "batched_columns", "clipped_centre"},
                (2, 12, 72): {"narrow_map", "batched_columns", "clipped_centre"},
                (2, 9, 80): {"narrow_map", "width_is_window", "batched_columns", "clipped_centre"},
                (2, 16, 65): {"narrow_map", "batched_columns", "clipped_centre"}}
    for case, got in reached.items():
        assert got & SPLAT_NEW == by_shape[case[1]] | ({"centre_unplaced"} if case[0] == "centre_bad" else set()), case
        assert "seam_window" in got, case
        if case[0] == "back":
            assert "negative_origin" in got, case

    def union(kind, shape=None, alpha=None):
        return set().union(*(g for c, g in reached.items() if c[0] == kind and shape in (None, c[1]) and alpha in (None, c[3])))

    # a map no wider than the window holds every column: no tap can leave it in x there
    assert {"direct_x", "split_pixel"} <= union("torn_x", (3, 20, 200), 0.0) and "direct_x" not in union("torn_x", (2, 12, 72))
    assert all({"direct_y", "split_pixel"} <= union("torn_y", s) for s in sr.DEVICE_SHAPES)
    assert {"direct_x", "direct_y", "split_pixel"} <= union("margin", (3, 20, 200))
    assert all({"direct_y", "split_pixel"} <= union("margin", s) for s in ((2, 12, 72), (2, 16, 65)))
    far = spc.reached(sr.CENTRE_FAR)
    assert {"centre_unplaced", "three_columns", "batched_columns"} <= far
    jobs = spc.case_inputs(*sr.CENTRE_FAR)
    counts = lp.splat_window_counts(jobs[0]["flow"], jobs[0]["tau"], 20, 200, jobs[0]["mask"])
    assert counts["unplaced_tiles"] == counts["tiles"] == 3 * 3 * 4                 # every centre lands in [2^28, 2^30): splatted, not placed
    q = np.float32(32) + np.float32(jobs[0]["tau"]) * jobs[0]["flow"][0, 0, 4, 32]
    assert lp.SPLAT_NEAR <= q < lp.SPLAT_FAR


def test_no_case_of_the_splat_sweep_reaches_them():
    """The flows of the sweep do not depend on alpha or C (only the masks do, and a mask cannot add a path): 189 input sets stand
    for its 1 080 cases.  What they do reach: seam windows and negative origins at every shape, direct taps in x and split pixels
    at (1, 64, 128) only (the smaller maps are narrower than the window), direct taps in y also where `poles` and `expand` tear the
    rows of a smaller map."""
    seen = {}
    for kind in sr.FAMILIES:
        for shape in sr.SHAPES:
            got = set().union(*(spc.reached((kind, shape, t, 0.0, 1, nj)) for t in sr.TS for nj in sr.NJOBS))
            assert not got & SPLAT_NEW, (kind, shape, got)
            seen[shape] = seen.get(shape, set()) | got
    assert seen[(1, 64, 128)] == {"direct_x", "direct_y", "split_pixel", "seam_window", "negative_origin"}
    assert all("direct_x" not in seen[s] and {"seam_window", "negative_origin"} <= seen[s] for s in sr.SHAPES[:2])
    assert all(B == 1 or W < lp.SPLAT_TILE_X for B, H, W in sr.SHAPES) and max(W for _, _, W in sr.SHAPES) == 2 * lp.SPLAT_TILE_X


# ---- grids with a fixed cap (DESIGN.md sections 13 and 14) ---------------------------------------------------------------------------
def test_capped_grid_constants_and_rules_are_those_of_the_sources():
    elem, aug = _text("pf_elem_kernels.hip"), _text("pf_augment.hip")
    assert "\nconstexpr int kBlock = 256;" in elem and "constexpr int kBlock = 256;\nconstexpr int kMaxBlocks = 1024;" in aug
    assert (lp.ELEM_BLOCK, lp.OS_MAX_BLOCKS, lp.AUG_MAX_BLOCKS, lp.AUG_ERASE_BLOCKS, lp.OS_SELECT_PER) == (256, 2048, 1024, 40, 8)
    assert "long blocks = (items + (long)kBlock * per - 1) / ((long)kBlock * per);" in elem
    assert "return blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);" in elem
    assert "pf_os_pass_kernel<0>, dim3((unsigned)pf_os_blocks(a.n, 8), (unsigned)a.B)" in elem
    assert "pf_os_pass_kernel<2>, dim3((unsigned)pf_os_blocks(a.n / 4, 1), (unsigned)a.B)" in elem
    assert "pf_os_pass_kernel<1>, dim3((unsigned)pf_os_blocks(a.n, 1), (unsigned)a.B)" in elem
    assert "pf_render_color_kernel<true>, dim3((unsigned)pf_os_blocks(a.n / 4, 1), (unsigned)a.B)" in elem
    assert "pf_render_color_kernel<false>, dim3((unsigned)pf_os_blocks(a.n, 1), (unsigned)a.B)" in elem
    assert "return r.W % 4 == 0 && ((uintptr_t)r.flow | (uintptr_t)r.len) % 16 == 0 && (uintptr_t)r.out % 4 == 0;" in elem
    for body in (_body(elem, "pf_os_pass_kernel"), _body(elem, "pf_render_color_kernel")):
        assert "stride = (long)gridDim.x * kBlock;" in body
        assert body.count("i += stride)") == 3 - (body.startswith("pf_render_color_kernel"))
    assert "long blocks = (items + kBlock - 1) / kBlock;" in aug
    assert "return (unsigned)(blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks));" in aug
    assert "pf_aug_contrast_kernel, dim3(pf_aug_blocks(N / 4), 2, (unsigned)B)" in aug
    assert "pf_aug_main_kernel<true>, dim3(pf_aug_blocks(N / 4), 3, (unsigned)B)" in aug
    assert "pf_aug_main_kernel<false>, dim3(pf_aug_blocks(N), 3, (unsigned)B)" in aug
    assert "pf_aug_erase_kernel, dim3(40, 2, (unsigned)B), dim3(kBlock)" in aug
    assert "const bool vec = W % 4 == 0 &&" in aug
    contrast, main, erase = (_body(aug, k) for k in ("pf_aug_contrast_kernel", "pf_aug_main_kernel", "pf_aug_erase_kernel"))
    assert "const long stride = (long)gridDim.x * kBlock;" in contrast and "i < N4; i += stride)" in contrast
    assert "const long stride = (long)gridDim.x * kBlock;" in main and main.count("i < items; i += stride)") == 2
    assert "for (int i = blockIdx.x * kBlock + threadIdx.x; i < total; i += gridDim.x * kBlock) {" in erase
    assert "const int total = w * h;" in erase
    h = _text("pf_augment.h")
    assert "w = r[2] < W - x0 ? r[2] : W - x0;" in h and "h = r[3] < H - y0 ? r[3] : H - y0;" in h


def test_capped_grid_rules_themselves():
    assert lp.os_grid(1, 8) == (1, 1, 1) and lp.os_grid(0, 1) == (1, 1, 1)
    assert lp.os_grid(512 * 1024, 8) == (256, 256, 8) and lp.os_grid(1000003, 8) == (489, 489, 8)      # 8 items per thread: 8 trips
    assert lp.os_grid(4194304, 8) == (2048, 2048, 8) and lp.os_grid(4194305, 8) == (2049, 2048, 9)
    assert lp.os_grid(524288, 1) == (2048, 2048, 1) and lp.os_grid(524289, 1) == (2049, 2048, 2)
    assert lp.aug_grid(262144) == (1024, 1024, 1) and lp.aug_grid(262145) == (1025, 1024, 2) and lp.aug_grid(0) == (1, 1, 1)
    assert lp.aug_erase_grid((0, 0, 128, 80), 100, 200) == (10240, 10240, 1)
    assert lp.aug_erase_grid((100, 50, 500, 500), 200, 300) == (200 * 150, 10240, 3)
    assert lp.aug_erase_grid((300, 0, 5, 5), 200, 300) is None and lp.aug_erase_grid((0, 0, 0, 5), 200, 300) is None


def test_the_capped_cases_reach_the_cap():
    """Every new case launches fewer workgroups than its items want, so some thread goes round its loop once more than in any
    older case: a ninth trip of a selection pass, a second trip of every kernel that takes one item per thread."""
    assert lp.os_grid(ck.OS_CAPPED_N, lp.OS_SELECT_PER) == (2051, 2048, 9)
    (H1, W1), (H4, W4) = ck.RENDER_CAPPED
    assert lp.render_grids(H1, W1) == {"one_pixel": (2050, 2048, 2)} and lp.render_grids(H4, W4) == {"four_pixel": (2052, 2048, 2)}
    assert H1 * W1 - 2048 * 256 == 484 and H4 * W4 // 4 - 2048 * 256 == 1024          # what the second trips hold
    (B4, H4, W4), (B1, H1, W1) = ac.CAPPED
    assert (B4, B1) == (1, 2)
    assert lp.augment_grids(H4, W4) == {"main_four_pixel": (1028, 1024, 2), "contrast": (1028, 1024, 2)}
    assert (H4 * W4 // 4 - 1024 * 256) * 4 == 2 * W4                                 # rows 512 and 513 are the second trip
    assert lp.augment_grids(H1, W1) == {"main_one_pixel": (1026, 1024, 2), "contrast": (257, 257, 1)}
    for B, H, W in ac.CAPPED:
        assert lp.aug_erase_grid(ac.CAPPED_RECT, H, W) == (12000, 10240, 2)


def test_no_older_case_reaches_a_cap():
    """The shapes of the tests that were there before (tests/test_hip_flow_viz.py, tests/test_hip_augment.py): none launches
    fewer workgroups than it wants, and no eraser rectangle holds more pixels than the 10 240 threads of its grid."""
    for n in (512 * 1024, 1, 7, 255, 29376, 1000003, 5):
        want, launched, trips = lp.os_grid(n, lp.OS_SELECT_PER)
        assert want == launched and trips <= lp.OS_SELECT_PER, n
    for H, W in fc.SIZES + ((64, 130), (512, 1024), (136, 216), (128, 256), (16, 32)):
        for g in list(lp.render_grids(H, W).values()) + [lp.os_grid(H * W, 1)]:           # an unaligned map: the one-pixel form
            assert g[0] == g[1] and g[2] == 1, (H, W)
    largest = 0
    for H, W in ac.SIZES + (ac.OP_SIZE, (5, 7), (512, 1024)):
        # the main kernel's one-pixel form at a width that is a multiple of 4 runs only at ac.SIZES[0] (unaligned outputs)
        for g in list(lp.augment_grids(H, W).values()) + [lp.aug_grid(H * W)] * ((H, W) == ac.SIZES[0]):
            assert g[0] == g[1] and g[2] == 1, (H, W)
        # the sampler draws both sides of a rectangle with randint(50, 100): at most 99 x 99, clipped by the map
        largest = max(largest, lp.aug_erase_grid((0, 0, 100, 100), H, W)[0])
        for _, rects, _, _ in ac.hand_cases(H, W):
            for r in rects:
                g = lp.aug_erase_grid(r, H, W)
                assert g is None or g[2] == 1, (H, W, r)
    assert largest == 10000 < lp.AUG_ERASE_BLOCKS * lp.ELEM_BLOCK
