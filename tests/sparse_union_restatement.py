"""The statement of sparse tensors on different key sets that the tests hold csrc/sparse_union.hip against, in numpy /
torch on the CPU: the union map and the prune map as np.union1d / np.searchsorted / np.nonzero, the two feature ops as index
expressions in float32.  Every comparison against it is ``torch.equal``: the maps are integers, a union row is one fp32 add or
subtract of two given floats, the gathers copy.  The four functions take and return what ``vdetr_amd.sparse_ops.union_map`` /
``prune_map`` / ``union_add`` / ``take_rows`` do, so the CPU wiring tests patch them in for those entry points."""
import numpy as np
import torch

KEY_BIAS = 32768


def pack(batch, x, y, z):
    """the key of a site (vdetr_amd.sparse_ops.pack_keys)"""
    return (int(batch) << 48) | ((int(x) + KEY_BIAS) << 32) | ((int(y) + KEY_BIAS) << 16) | (int(z) + KEY_BIAS)


def union_map(a_keys, b_keys):
    a, b = a_keys.cpu().numpy(), b_keys.cpu().numpy()
    u = np.union1d(a, b).astype(np.int64)
    row_a, row_b = np.searchsorted(u, a).astype(np.int32), np.searchsorted(u, b).astype(np.int32)
    src_a, src_b = np.full(len(u), -1, np.int32), np.full(len(u), -1, np.int32)
    src_a[row_a] = np.arange(len(a), dtype=np.int32)
    src_b[row_b] = np.arange(len(b), dtype=np.int32)
    return tuple(torch.from_numpy(v) for v in (u, row_a, row_b, src_a, src_b))


def prune_map(mask, keys):
    m, k = mask.cpu().numpy(), keys.cpu().numpy()
    kept = np.nonzero(m)[0].astype(np.int32)
    pos = np.full(len(m), -1, np.int32)
    pos[kept] = np.arange(len(kept), dtype=np.int32)
    return torch.from_numpy(kept), torch.from_numpy(pos), torch.from_numpy(k[kept].astype(np.int64))


def _spread(f, row, n):
    """f's rows at their places in a table of n rows of zeros (differentiable: the gradient of f is the gather through row)"""
    return torch.zeros((n, f.shape[1]), dtype=f.dtype).index_copy(0, row.long(), f)


def union_add(fa, fb, row_a, row_b, src_a, src_b, sign=1):
    nu = src_a.shape[0]
    a, b = _spread(fa, row_a, nu), _spread(fb, row_b, nu)
    return a + b if sign > 0 else a - b


def take_rows(x, idx, back=None, sign=1):
    """y[r] = sign * x[idx[r]], an exact zero where idx[r] < 0 (``back`` is what the device op's backward gathers through: the
    autograd of this expression states the same gradient)"""
    if x.shape[0] == 0:
        return torch.zeros((idx.shape[0], x.shape[1]), dtype=x.dtype)
    rows = x[idx.long().clamp(min=0)]
    rows = -rows if sign < 0 else rows
    return torch.where((idx >= 0)[:, None], rows, torch.zeros_like(rows))


def route_to_cpu(mp):
    """the native entry points of vdetr_amd.sparse_ops on CPU tensors: the convolution's six go to oracle/sparse_oracle.py (as the
    ``cpu_sparse_ops`` fixture of tests/test_oracle_sparse.py routes them), the four of this file's subject to the functions above"""
    from oracle import sparse_oracle as O
    from vdetr_amd import sparse_ops as S

    def gather_sum(d, inv, offset_major=False, flat=False):
        if flat:  # rows of a flat [P, C] source: present it as [P, K, C] with the row repeated along K
            return O.gather_sum(d[:, None, :].expand(-1, inv.shape[0], -1), inv)
        return O.gather_sum(d.permute(1, 0, 2) if offset_major else d, inv)

    mp.setattr(S, "kernel_map", lambda ik, ok, off: O.kernel_map(ik, ok, off))
    mp.setattr(S, "inverse_map", lambda nbr, nin: O.inverse_map(nbr, nin))
    mp.setattr(S, "gather_cols", lambda f, nbr: O.gather_cols(f, nbr).contiguous())
    mp.setattr(S, "gather_sum", gather_sum)
    mp.setattr(S, "pairs_gemm", lambda x, arow, w, plan, tr: O.pairs_gemm(x, arow, w, plan.seg, tr))
    mp.setattr(S, "pairs_wgrad", lambda x, dy, plan, cin, cout: O.pairs_wgrad(x, dy, plan.pin, plan.pout, plan.seg, plan.K))
    mp.setattr(S, "union_map", union_map)
    mp.setattr(S, "prune_map", prune_map)
    mp.setattr(S, "union_add", union_add)
    mp.setattr(S, "take_rows", take_rows)
    return S


# ---- brute force: what the restatement itself is held against on small key lists --------------------------------------------------
def brute_union(a, b):
    """(u, row_a, row_b, src_a, src_b) of two lists of distinct ints by set arithmetic and list.index"""
    u = sorted(set(a) | set(b))
    return (u, [u.index(k) for k in a], [u.index(k) for k in b], [a.index(k) if k in a else -1 for k in u],
            [b.index(k) if k in b else -1 for k in u])


def brute_prune(mask, keys):
    kept = [i for i, m in enumerate(mask) if m]
    return kept, [kept.index(i) if m else -1 for i, m in enumerate(mask)], [keys[i] for i in kept]


# ---- key sets of the GPU tests ----------------------------------------------------------------------------------------------------
RELATIONS = ("disjoint", "identical", "a_in_b", "b_in_a", "interleaved", "a_below_b", "two_scenes", "three_scenes")


def key_sets(relation, na, nb, seed=0):
    """sorted unique int64 key tensors (a [na], b [nb]) in the given relation (where a relation fixes one size from the other —
    identical, a subset — the larger of the two counts is the superset's)"""
    rng = np.random.default_rng(seed + 1000 * na + nb)

    def draw(n, lo=0, hi=1 << 40):
        if n == 0:
            return np.zeros(0, np.int64)
        k = np.unique(rng.integers(lo, hi, 3 * n + 8, dtype=np.int64))
        return np.sort(rng.permutation(k)[:n])

    def mixed(a, nb, scenes):
        """a on even low words, b = a share of a's keys + private keys on odd ones: exactly nb keys"""
        if scenes > 1:  # spread over the batch bits
            a = np.sort(a | (rng.integers(0, scenes, len(a), dtype=np.int64) << 48))
        share = a[::3][:nb // 3]
        private = draw(nb - len(share), 0, 1 << 20) * 2 + 1
        if scenes > 1:
            private = private | (rng.integers(0, scenes, len(private), dtype=np.int64) << 48)
        return a, np.sort(np.concatenate((share, private)))

    if relation == "disjoint":
        pool = draw(na + nb)
        pick = rng.permutation(len(pool))
        a, b = np.sort(pool[pick[:na]]), np.sort(pool[pick[na:na + nb]])
    elif relation == "identical":
        a = draw(max(na, nb))
        b = a.copy()
    elif relation in ("a_in_b", "b_in_a"):
        big, small = max(na, nb), min(na, nb)
        sup = draw(big)
        sub = np.sort(rng.permutation(sup)[:small])
        a, b = (sub, sup) if relation == "a_in_b" else (sup, sub)
    elif relation == "interleaved":
        a, b = mixed(draw(na, 0, 1 << 20) * 2, nb, 1)
    elif relation == "a_below_b":
        a, b = draw(na, 0, 1 << 30), draw(nb, 1 << 31, 1 << 40)
    else:
        a, b = mixed(draw(na, 0, 1 << 20) * 2, nb, 2 if relation == "two_scenes" else 3)
    assert (np.diff(a) > 0).all() and (np.diff(b) > 0).all()
    return torch.from_numpy(a.astype(np.int64)), torch.from_numpy(b.astype(np.int64))


def run_across_boundary(tile, run=9):
    """two key sets that share a run of ``run`` consecutive keys whose positions straddle a multiple of ``tile`` in BOTH: a holds
    tile - run // 2 private keys below the run, b holds tile + tile - run // 2 (so the run crosses a's first and b's second tile
    boundary), and both continue with private keys above it"""
    lo = run // 2
    a_low = np.arange(tile - lo, dtype=np.int64) * 4            # ≡ 0 mod 4
    b_low = np.arange(2 * tile - lo, dtype=np.int64) * 4 + 1     # ≡ 1 mod 4
    base = 16 * tile
    shared = base + np.arange(run, dtype=np.int64) * 4 + 2
    a_high = base + 1000 + np.arange(tile // 2 + 3, dtype=np.int64) * 4
    b_high = base + 1000 + np.arange(tile // 3 + 1, dtype=np.int64) * 4 + 1
    a = np.concatenate((a_low, shared, a_high))
    b = np.concatenate((b_low, shared, b_high))
    assert (np.diff(a) > 0).all() and (np.diff(b) > 0).all()
    return torch.from_numpy(a), torch.from_numpy(b)


def scene_keys(counts, seed=0):
    """sorted keys of len(counts) scenes with the given site counts (scene s in the batch bits)"""
    rng = np.random.default_rng(seed)
    parts = []
    for s, n in enumerate(counts):
        k = np.unique(rng.integers(0, 1 << 40, 3 * n + 8, dtype=np.int64))
        parts.append(np.sort(rng.permutation(k)[:n]) | (np.int64(s) << 48))
    return torch.from_numpy(np.concatenate(parts).astype(np.int64))


MASKS = ("all", "none", "first", "last", "middle", "alternating", "no_middle_scene", "no_last_scene")


def scene_split(n):
    """three scene sizes adding up to n (n >= 3), otherwise one scene"""
    return [n] if n < 3 else [n // 3, n // 3, n - 2 * (n // 3)]


def mask_of(kind, counts):
    n = sum(counts)
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "middle":
        m[n // 2] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind in ("no_middle_scene", "no_last_scene"):
        m[:] = True
        s = 1 if kind == "no_middle_scene" else len(counts) - 1
        start = sum(counts[:s])
        m[start:start + counts[s]] = False
    return torch.from_numpy(m)
