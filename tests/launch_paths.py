"""The launch rules of csrc/pf_segments.hip and csrc/pf_tracker.hip that exist only on the device, restated as pure functions
(DESIGN.md sections 25 and 26): the grids of pf_seg_objects_accumulate and pf_trk_vote_kernel, which are capped by the CU count and
walk what is left in further trips of their loops, and the rows a thread of pf_seg_rank_scan holds.  tests/test_launch_paths.py pins
every constant and rule below to the text of the sources; the device tests use them to say which path a case reaches on the card at
hand.  Not collected."""

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
