"""Constructed inputs for csrc/nms_bitmask.h's greedy scan that the tests of its three callers share (rpn, det_post, umr_nms): boxes
64 wide and 32 high on one line, given by their left edge q -- (q, 0, q + 64, 32) -- in rank order.  Two such boxes d apart have
IoU (64 - d) / (64 + d), exact in float32: 1 at d = 0, 0.6 at d = 16, 1/3 at d = 32, 0 from d = 64 on; nothing is near the 0.5 threshold.
The scan walks the ranks 64 at a time, so the cases are placed by block (rank // 64)."""
import numpy as np

F32 = np.float32
THRESH = 0.5
WIDTH, HEIGHT = 64, 32

# chains: A suppresses B, B alone would suppress C, A does not suppress C -- C is kept
CHAIN_IN_ONE_BLOCK = (3, 10, 40)                   # A, B, C in block 0
CHAIN_INTO_THE_NEXT = (60, 70, 90)                 # A in block 0, B and C in block 1
CHAIN_OVER_A_BLOCK = (100, range(128, 192), 200)   # A in block 1, all of block 2 are B (the block is skipped whole), C in block 3
DUPLICATES = range(256, 320)                       # block 4: 64 times the same box, the first is kept
ZERO_AREA = (320, 321)                             # two identical boxes of width 0: 0 / 0 is a NaN and suppresses nothing
N_RANKS = 322


def line_boxes(q, width=WIDTH):
    q = np.asarray(q, F32)
    return np.stack([q, np.zeros_like(q), q + np.asarray(width, F32),np.full_like(q, HEIGHT)], axis=1).astype(F32)


def constructed(zero_area=True):
    """(left edges [n], widths [n], the ranks a greedy NMS at THRESH keeps) -- n = 322, or 320 without the zero-area pair"""
    n = N_RANKS if zero_area else N_RANKS - 2
    q = 1000 + 128 * np.arange(n)                  # every other rank: a box of its own, 128 from the next
    width = np.full(n, WIDTH)
    gone = []
    for base, (a, b, c) in ((0, CHAIN_IN_ONE_BLOCK), (200, CHAIN_INTO_THE_NEXT), (400, CHAIN_OVER_A_BLOCK)):
        b = [b] if isinstance(b, int) else list(b)
        q[a], q[b], q[c] = base, base + 16, base + 32
        gone += b
    q[list(DUPLICATES)] = 700
    gone += list(DUPLICATES)[1:]
    if zero_area:
        q[list(ZERO_AREA)], width[list(ZERO_AREA)] = 900, 0
    kept = [r for r in range(n) if r not in set(gone)]
    return q, width, kept


def constructed_boxes(zero_area=True):
    q, width, kept = constructed(zero_area)
    return line_boxes(q, width), kept


def check_expected(kept, zero_area=True):
    """what the cases are there for, on a kept list that a restatement or a device produced"""
    kept = list(kept)
    assert kept == constructed(zero_area)[2]
    for a, b, c in (CHAIN_IN_ONE_BLOCK, CHAIN_INTO_THE_NEXT, CHAIN_OVER_A_BLOCK):
        b = [b] if isinstance(b, int) else list(b)
        assert a in kept and c in kept and not set(b) & set(kept)
    assert [r for r in kept if r in DUPLICATES] == [DUPLICATES[0]]
    assert not zero_area or set(ZERO_AREA) <= set(kept)
