"""The launch rules of tests/launch_paths.py are those of the sources, and the cases built on them reach what they are there for
(DESIGN.md sections 25 and 26): every constant and rule is pinned to the text of csrc/pf_segments.hip, csrc/pf_tracker.hip and
csrc/pf_tracker.h, so a change in a launcher has to be noticed here; sc.DEVICE_PATHS and tc.DEVICE_PATHS reach their paths on cards
of 32, 64, 256 and 304 CUs; no shape of sc.SWEEP or tc.SHAPES reaches any of them on a whole MI355X."""
import os
import re

import launch_paths as lp
import segments_cases as sc
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
