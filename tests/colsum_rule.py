"""TEST INFRASTRUCTURE: the fixed-order column sums of cdsegnet_amd/csrc/colsum.h restated in plain Python - the row partition
and workspace size (BatchNorm: 256 rows a block at least; the fusion gate and the skip statistics: 64) and the order in which
one column's rows are added on the vector path.  Never imported by the product."""
MIN_ROWS_BN, MIN_ROWS_SWEEP = 256, 64


def partition(rows, min_rows):
    """(rows_per_block, blocks): at most 256 blocks of at least `min_rows` rows, a multiple of 64 beyond that; no empty block."""
    rpb = -(-rows // 256)
    rpb = min_rows if rpb < min_rows else -(-rpb // 64) * 64
    return rpb, (-(-rows // rpb) if rows > 0 else 0)


def ws_bytes(rows, nsums, c, min_rows):
    """blocks x nsums x c doubles."""
    return partition(rows, min_rows)[1] * nsums * c * 8 if rows > 0 else 0


def ordered_sum(column, c, min_rows, segs):
    """The fp64 sum of one column (a sequence of Python floats, one per row) in the documented order for width c (a multiple
    of 4, the vector path): R = 256 // (c // 4) row slots a block; slot r adds the block's rows r, r + R, .. by ascending
    index; the slots are added by ascending slot; the block partials by ascending block inside each of `segs` segments of
    ceil(blocks / segs) consecutive blocks, then the segment sums by ascending segment (segs = 1: one chain)."""
    rpb, blocks = partition(len(column), min_rows)
    R = 256 // (c // 4)
    partials = []
    for b in range(blocks):
        rows = column[b * rpb:(b + 1) * rpb]
        slots = []
        for r in range(R):
            t = 0.0
            for v in rows[r::R]:
                t += v
            slots.append(t)
        t = slots[0]
        for v in slots[1:]:
            t += v
        partials.append(t)
    seg = -(-blocks // segs)
    sums = []
    for g in range(0, blocks, seg):
        t = partials[g]
        for v in partials[g + 1:g + seg]:
            t += v
        sums.append(t)
    t = sums[0]
    for v in sums[1:]:
        t += v
    return t
