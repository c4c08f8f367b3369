"""Restatements of the bytes that the launches with a bare workspace pointer touch, written from the kernels' own indexing:
the grid of the launch that writes times the footprint of one workgroup, plus whatever sits behind the partials.  The size
functions of the library (`vdetr_*_workspace_bytes`, `vdetr_sp_pair_plan_workspace_ints`) have to answer at least this much;
they may answer more (a bound that grows with N where the count itself does not).  Nothing here imports ``vdetr_amd``.

  sp_bn.hip      a workgroup per bn_rows(N) rows writes [3][C] floats (forward) or [2][C] (backward) at index * 3 C resp.
                 index * 2 C; the backward's finalize writes [2][C] sums at nblk * 3 C
  sp_inorm.hip   grid = ceil(N / stat_rows(N)) + nseg workgroups (those past the last chunk return), [3][C] resp. [2][C] floats each
  heads.hip      two tables of [B N / 32 tiles][G * 256 channels][2] floats; the merge launch writes entry 0 of a table
  add_ln.hip     a workgroup per 16 rows writes up to [4][C] floats at index * 4 C
  pack.hip       the split column sum: [n][S][cols] floats, S = the row splits
  sparse_conv.hip (pair plan)  [K][ceil(nout / 256)] ints
"""
F4 = 4  # bytes of a float / an int


def ceil_div(a, b):
    return -(-a // b)


def round16(r):
    return ceil_div(r, 16) * 16


def bn_rows(N):
    """rows per workgroup of sp_bn.hip: N / 1024, kept in 16 .. 128, rounded up to a multiple of 16"""
    return round16(min(max(N // 1024, 16), 128))


def sp_bn_need(N, C):
    if N <= 0 or C <= 0:
        return 0  # (nothing is launched)
    nblk = ceil_div(N, bn_rows(N))
    forward = nblk * 3 * C
    backward = max(nblk * 2 * C, nblk * 3 * C + 2 * C)  # the partials, and the two sums behind the forward's partials
    return max(forward, backward) * F4


def inorm_stat_rows(N):
    """rows per statistics chunk of sp_inorm.hip: ceil(N / 64), at least 16, rounded up to a multiple of 16"""
    return round16(max(ceil_div(N, 64), 16))


def sp_inorm_need(N, C, nseg):
    if N <= 0 or C <= 0 or nseg <= 0:
        return 0
    grid = ceil_div(N, inorm_stat_rows(N)) + nseg
    return grid * 3 * C * F4


def inorm_chunks(sizes, rows):
    """the chunks a batch of scenes really has: every scene is cut on its own"""
    return sum(ceil_div(n, rows) for n in sizes)


def heads_need(B, N, G):
    if B <= 0 or N <= 0 or G <= 0:
        return 0
    tiles = B * N // 32
    return 2 * tiles * G * 256 * 2 * F4


def add_ln_bwd_need(rows, C):
    if rows <= 0 or C <= 0:
        return 0
    return ceil_div(rows, 16) * 4 * C * F4


def colsum_splits(n, rows, cols):
    """row splits of the four-columns-per-lane kernel: doubled towards 512 workgroups while a split keeps 32 rows"""
    if cols % 4:
        return 1
    wgs = n * ceil_div(cols, 256)
    S = 1
    while wgs * S < 512 and S < 256 and rows // (2 * S) >= 32:
        S *= 2
    return S


def colsum_need(n, rows, cols):
    if n <= 0 or rows <= 0 or cols <= 0:
        return 0
    S = colsum_splits(n, rows, cols)
    return n * S * cols * F4 if S > 1 else 0


def pair_plan_need_ints(K, nout):
    if K <= 0 or nout <= 0:
        return 0
    return K * ceil_div(nout, 256)


def steps(rule, lo, hi):
    """every N in lo + 1 .. hi at which rule(N) differs from rule(N - 1)"""
    out, prev = [], rule(lo)
    for N in range(lo + 1, hi + 1):
        cur = rule(N)
        if cur != prev:
            out.append(N)
        prev = cur
    return out


def sweep(rules, hi=70000, dense=2100):
    """the values of N a size function is swept over: 0 .. dense, every step of the rules and one either side of it, one either
    side of the multiples of 16, 32, 64 and 128 next to a step, a coarse grid, hi"""
    ns = set(range(0, dense + 1)) | set(range(0, hi + 1, 997)) | {hi - 1, hi}
    for rule in rules:
        for s in steps(rule, 0, hi):
            for m in (1, 16, 32, 64, 128, 256):
                base = s // m * m
                ns.update((base - m - 1, base - m, base - 1, base, base + 1, base + m, base + m + 1, s - 1, s, s + 1))
    return sorted(n for n in ns if 0 <= n <= hi)
