"""The launch rules of csrc/pf_segments.hip and csrc/pf_tracker.hip that exist only on the device, restated as pure functions
(DESIGN.md sections 25 and 26): the grids of pf_seg_objects_accumulate and pf_trk_vote_kernel, which are capped by the CU count and
walk what is left in further trips of their loops, and the rows a thread of pf_seg_rank_scan holds.  Likewise the LDS window of
pf_splat_acc_kernel (csrc/pf_splat.hip) and the grids with a fixed cap of the order statistic, the render
(pf_os_blocks, section 13) and the augmentor (pf_aug_blocks and the eraser's 40 workgroups, section 14).
tests/test_launch_paths.py pins every constant and rule below to the text of the sources; the device tests use them to say which
path a case reaches on the card at hand.  Not collected."""
import numpy as np


K_FLAT = 1024                 # pf_segments.hip kFlat: threads, and pixels per trip, of an accumulate workgroup
K_LDS_OBJECTS = 512           # pf_segments.hip kLdsObjects: M up to which the accumulate kernel keeps its partial sums in LDS
K_SCAN_BLOCK = 256            # pf_segments.hip kBlock: threads of pf_seg_rank_scan's one workgroup per image
K_VOTE = 1024                 # pf_tracker.hip kVote: threads of a vote workgroup
K_VOTE_WAVES = K_VOTE // 64   # items (64 pixels of one row) per trip of a vote workgroup
TK_LDS_OBJECTS = 64           # pf_tracker.h PF_TK_LDS_OBJECTS: M up to which the vote kernel keeps its partial matrix in LDS
SEG_MAX_OBJECTS = 4096        # PF_SEG_MAX_OBJECTS
TRK_MAX_OBJECTS = 256         # PF_TRK_MAX_OBJECTS = threads of pf_trk_match_kernel
CU_COUNTS = (32, 64, 256, 304)          # a partition of a card, ..., a whole MI355X, a larger card


def _ceil(a, b):
    return (a + b - 1) // b


def cap(B, cus):
    """cap = (2L * cus + B - 1) / B: two workgroups per CU in all, shared by the B images, at least one each."""
    return _ceil(2 * cus, B)


def seg_accumulate_grid(B, H, W, cus):
    """(workgroups wanted, workgroups launched) per image of pf_seg_objects_accumulate."""
    want = _ceil(H * W, K_FLAT)
    return want, min(want, cap(B, cus))


def trk_vote_grid(B, H, W, cus):
    """(workgroups wanted, workgroups launched) per image of pf_trk_vote_kernel: an item is 64 pixels of one row."""
    want = _ceil(H * _ceil(W, 64), K_VOTE_WAVES)
    return want, min(want, cap(B, cus))


def trips(grid):
    """The trips of the loop that the busiest workgroup of a (wanted, launched) grid makes."""
    want, launched = grid
    return _ceil(want, launched)


def second_trip(grid):
    """Does some workgroup of a (wanted, launched) grid go round its loop again?"""
    return trips(grid) > 1


def seg_scan_rows_per_thread(H):
    """per = (H + kBlock - 1) / kBlock of pf_seg_rank_scan."""
    return _ceil(H, K_SCAN_BLOCK)


def seg_scan_rows_of_thread(H, t):
    """The rows thread t of the scan really holds: [min(t per, H), min(t per + per, H))."""
    per = seg_scan_rows_per_thread(H)
    return min(t * per + per, H) - min(t * per, H)


def clipped_threads(H):
    """The threads of the scan that hold fewer than `per` rows, as a range: the first may hold some, the others hold none."""
    per = seg_scan_rows_per_thread(H)
    return range(H // per, K_SCAN_BLOCK)


def seg_device_paths(B, C, H, W, M, cus):
    """The device-only paths of DESIGN.md section 25 that one update reaches, as a set of names."""
    out = set()
    if second_trip(seg_accumulate_grid(B, H, W, cus)):
        out.add("accumulate_second_trip_lds" if M <= K_LDS_OBJECTS else "accumulate_second_trip_global")
    if seg_scan_rows_per_thread(H) > 1:
        out.add("scan_two_rows_per_thread")
        if len(clipped_threads(H)):
            out.add("scan_clipped_threads")
    if M in (K_LDS_OBJECTS, SEG_MAX_OBJECTS):
        out.add(f"table_{M}")
    return out


def trk_device_paths(B, H, W, M, cus):
    """The same for a push of the tracker."""
    out = set()
    if second_trip(trk_vote_grid(B, H, W, cus)):
        out.add("vote_second_trip_lds" if M <= TK_LDS_OBJECTS else "vote_second_trip_global")
    if M == TRK_MAX_OBJECTS:
        out.add(f"table_{M}")
    return out


def describe_seg(B, C, H, W, cus):
    g = seg_accumulate_grid(B, H, W, cus)
    per = seg_scan_rows_per_thread(H)
    cl = clipped_threads(H)
    return (f"{B}x{C}x{H}x{W} on {cus} CUs: accumulate grid {g[1]} of {g[0]} wanted per image, {trips(g)} trip(s); scan {per} row(s) per "
            f"thread, " + (f"threads {cl[0]}.. clipped (thread {cl[0]} holds {seg_scan_rows_of_thread(H, cl[0])})" if per > 1 and len(cl)
                           else "no thread clipped" if per > 1 else f"the threads from {H} idle"))


def describe_trk(B, H, W, cus):
    g = trk_vote_grid(B, H, W, cus)
    return f"{B}x{H}x{W} on {cus} CUs: vote grid {g[1]} of {g[0]} wanted per image, {trips(g)} trip(s)"


# ---- pf_splat_acc_kernel: the LDS window (csrc/pf_splat.hip) ---------------------------------------------------------------------
SPLAT_TILE_Y, SPLAT_TILE_X = 8, 64            # kTileY, kTileX: source pixels of a workgroup
SPLAT_MARGIN_Y, SPLAT_MARGIN_X = 4, 8         # kMarginY, kMarginX
SPLAT_WIN_Y, SPLAT_WIN_X = SPLAT_TILE_Y + 2 * SPLAT_MARGIN_Y, SPLAT_TILE_X + 2 * SPLAT_MARGIN_X        # kWinY, kWinX: 16 x 80
SPLAT_NEAR = 2.0 ** 28                        # kNear: a window is placed only this near to the map
SPLAT_FAR = 2.0 ** 30                         # pf_splat.h PF_SPLAT_FAR: a landing at or beyond it is skipped
SPLAT_PATHS = ("centre_unplaced", "narrow_map", "width_is_window", "batched_columns", "three_columns", "clipped_centre", "direct_x",
               "direct_y", "split_pixel", "seam_window", "negative_origin")


def splat_window_counts(flow, tau, H, W, skip=None):
    """What one job of pf_splat_acc_kernel does with its window, in the kernel's own fp32 steps.  flow [B,2,H,W] (or [2,H,W])
    float32, tau the job's; skip [B,H,W]: pixels the kernel leaves out for another reason (mask, a value or metric that is not
    finite).  Returns counts: tiles whose centre is not placed, tiles whose window straddles the seam, tiles whose origin is
    negative before the %, taps into the window, taps that go to memory directly because of their column / their row, pixels whose
    taps split between the two; and the facts of the shape (tile columns, images)."""
    f = np.asarray(flow, np.float32)
    f = f[None] if f.ndim == 3 else f
    B = f.shape[0]
    assert f.shape[1:] == (2, H, W)
    tau = np.float32(tau)
    skip = np.zeros((B, H, W), bool) if skip is None else (np.asarray(skip).reshape(B, H, W) != 0)
    y, x = np.mgrid[0:H, 0:W]
    with np.errstate(invalid="ignore", over="ignore"):
        qx = x.astype(np.float32) + tau * f[:, 0]
        qy = y.astype(np.float32) + tau * f[:, 1]
        assert qx.dtype == np.float32
        # the tile of every pixel, its centre pixel, where that lands, and the window's origin
        ty0, tx0 = y // SPLAT_TILE_Y * SPLAT_TILE_Y, x // SPLAT_TILE_X * SPLAT_TILE_X
        cy, cx = np.minimum(ty0 + SPLAT_TILE_Y // 2, H - 1), np.minimum(tx0 + SPLAT_TILE_X // 2, W - 1)
        cqx, cqy = qx[:, cy, cx], qy[:, cy, cx]
        ok = (np.abs(cqx) < np.float32(SPLAT_NEAR)) & (np.abs(cqy) < np.float32(SPLAT_NEAR))       # a NaN compares false
        ix = np.where(ok, np.floor(np.where(ok, cqx, 0)).astype(np.int64), cx)
        iy = np.where(ok, np.floor(np.where(ok, cqy, 0)).astype(np.int64), cy)
        oy = iy - (cy - ty0) - SPLAT_MARGIN_Y
        raw = ix - (cx - tx0) - SPLAT_MARGIN_X
        ox = np.mod(raw, W)                                        # C's % and the fix-up of a negative remainder
        live = (np.abs(qx) < np.float32(SPLAT_FAR)) & (np.abs(qy) < np.float32(SPLAT_FAR)) & ~skip
        qx, qy = np.where(live, qx, np.float32(0)), np.where(live, qy, np.float32(0))
    x0f, y0f = np.floor(qx), np.floor(qy)
    fx, fy = qx - x0f, qy - y0f
    gx, gy = np.float32(1) - fx, np.float32(1) - fy
    x0, y0 = np.mod(x0f.astype(np.int64), W), y0f.astype(np.int64)
    n_win = np.zeros((B, H, W), np.int64)
    n_dx, n_dy = np.zeros_like(n_win), np.zeros_like(n_win)
    for dy, by in ((0, gy), (1, fy)):
        for dx, bx in ((0, gx), (1, fx)):
            yy, xx = y0 + dy, np.mod(x0 + dx, W)
            tap = live & (bx * by > 0) & (yy >= 0) & (yy < H)
            xr = xx - ox
            xr = np.where(xr < 0, xr + W, xr)
            yr = yy - oy
            in_x, in_y = (xr >= 0) & (xr < SPLAT_WIN_X), (yr >= 0) & (yr < SPLAT_WIN_Y)
            n_win += tap & in_x & in_y
            n_dx += tap & ~in_x
            n_dy += tap & ~in_y
    first = (y == ty0) & (x == tx0)                                 # one pixel per tile
    direct = (n_dx + n_dy) > 0
    return dict(images=B, tile_columns=_ceil(W, SPLAT_TILE_X), tiles=int(first.sum()) * B,
                unplaced_tiles=int((~ok & first).sum()), seam_tiles=int(((ox + SPLAT_WIN_X > W) & first).sum()),
                negative_origins=int(((raw < 0) & first).sum()), clipped_centres=int(((tx0 + SPLAT_TILE_X // 2 > W - 1) & first).sum()),
                window_taps=int(n_win.sum()), direct_x_taps=int(n_dx.sum()), direct_y_taps=int(n_dy.sum()),
                split_pixels=int((direct & (n_win > 0)).sum()))


def splat_window_paths(flow, tau, H, W, skip=None):
    """The device-only paths of pf_splat_acc_kernel that one job reaches, as a set of the names in SPLAT_PATHS."""
    c = splat_window_counts(flow, tau, H, W, skip)
    cols = c["tile_columns"]
    facts = dict(centre_unplaced=c["unplaced_tiles"], narrow_map=cols >= 2 and W <= SPLAT_WIN_X, width_is_window=W == SPLAT_WIN_X,
                 batched_columns=c["images"] > 1 and cols > 1, three_columns=cols > 2, clipped_centre=c["clipped_centres"],
                 direct_x=c["direct_x_taps"], direct_y=c["direct_y_taps"], split_pixel=c["split_pixels"], seam_window=c["seam_tiles"],
                 negative_origin=c["negative_origins"])
    assert set(facts) == set(SPLAT_PATHS)
    return {k for k, v in facts.items() if v}


def splat_case_paths(jobs, H, W):
    """The union over the jobs of a case (dicts of tests/splat_ref.py: flow, tau, mask)."""
    return set().union(*(splat_window_paths(q["flow"], q["tau"], H, W, q["mask"]) for q in jobs))


# ---- grids with a fixed cap: pf_os_blocks (csrc/pf_elem_kernels.hip), pf_aug_blocks and the eraser (csrc/pf_augment.hip) -------------
ELEM_BLOCK = 256              # kBlock of both files
OS_MAX_BLOCKS = 2048          # pf_os_blocks: at most 2048 workgroups per image
OS_SELECT_PER = 8             # items per thread of a selection pass (launch_os_pass); the length and colour kernels take 1
AUG_MAX_BLOCKS = 1024         # pf_augment.hip kMaxBlocks
AUG_ERASE_BLOCKS = 40         # workgroups per rectangle of pf_aug_erase_kernel


def _capped(items, per_block, cap):
    want = max(1, _ceil(items, per_block))
    launched = min(want, cap)
    return want, launched, max(1, _ceil(items, launched * ELEM_BLOCK))


def os_grid(items, per):
    """(workgroups wanted, launched, trips of a thread's loop) of pf_os_blocks(items, per): the loop's stride is the launched
    threads, whatever `per` says."""
    return _capped(items, ELEM_BLOCK * per, OS_MAX_BLOCKS)


def aug_grid(items):
    """The same of pf_aug_blocks(items)."""
    return _capped(items, ELEM_BLOCK, AUG_MAX_BLOCKS)


def aug_erase_grid(rect, H, W):
    """(threads wanted = pixels of the clipped rectangle, threads launched, trips) of pf_aug_erase_kernel for (x0, y0, dx, dy);
    None when pf_aug_rect refuses the rectangle."""
    x0, y0, dx, dy = rect
    if x0 < 0 or x0 >= W or y0 < 0 or y0 >= H or dx <= 0 or dy <= 0:
        return None
    total = min(dx, W - x0) * min(dy, H - y0)
    launched = AUG_ERASE_BLOCKS * ELEM_BLOCK
    return total, launched, max(1, _ceil(total, launched))


def render_grids(H, W):
    """{kernel form: grid} of pf_flow_render at H x W: the four-pixel forms when W % 4 == 0 (and the maps are aligned), else the
    one-pixel forms; the length pass and the colour kernel launch the same grid."""
    return {"four_pixel": os_grid(H * W // 4, 1)} if W % 4 == 0 else {"one_pixel": os_grid(H * W, 1)}


def augment_grids(H, W):
    """{kernel: grid} of pf_augment_360 at H x W: the contrast pass always walks quads; the main kernel as render_grids."""
    main = {"main_four_pixel": aug_grid(H * W // 4)} if W % 4 == 0 else {"main_one_pixel": aug_grid(H * W)}
    return dict(main, contrast=aug_grid(H * W // 4))
