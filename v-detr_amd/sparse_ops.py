"""Sparse-convolution primitives of the backbone on top of lib/libvdetr_hip.so.

A sparse tensor is a sorted int64 KEY vector [N] (``pack_keys``: batch, x, y, z as biased 16-bit fields, so ascending key
order is lexicographic coordinate order) plus a point-major feature table [N, C] — the layout the hot path's FPS and row
gathers consume.  The four native entry points (kernel map, inverse map, column gather, adjoint gather: csrc/sparse_conv.hip)
are geometry / HBM-stream kernels; the contraction itself is ONE library GEMM per layer over the gathered columns
(``col [N, K*Cin] @ W [K*Cin, Cout]``), its two gradients two more.  No CPU path: every entry point raises on CPU tensors.
"""
import ctypes
import os
import threading

import numpy as np
import torch
from torch.autograd import Function

from . import _lib as L

KEY_BIAS = 32768


def pack_keys(coords, check=True):
    """[N,4] integer (batch, x, y, z) -> int64 keys (include/vdetr_hip.h: vdetr_sp_kernel_map_i32).  ``check`` validates the
    16-bit field range (a device->host sync: used on the raw input coordinates only)."""
    c = coords.to(torch.int64)
    if check and c.numel():
        lo, hi = int(c[:, 1:].min()), int(c[:, 1:].max())
        if lo < -KEY_BIAS or hi >= KEY_BIAS or int(c[:, 0].min()) < 0 or int(c[:, 0].max()) >= 32768:
            raise ValueError(f"voxel coordinates outside the 16-bit key range: [{lo}, {hi}]")
    return (c[:, 0] << 48) | ((c[:, 1] + KEY_BIAS) << 32) | ((c[:, 2] + KEY_BIAS) << 16) | (c[:, 3] + KEY_BIAS)


def unpack_keys(keys):
    """int64 keys -> [N,4] int32 (batch, x, y, z)."""
    b = keys >> 48
    x = ((keys >> 32) & 0xFFFF) - KEY_BIAS
    y = ((keys >> 16) & 0xFFFF) - KEY_BIAS
    z = (keys & 0xFFFF) - KEY_BIAS
    return torch.stack((b, x, y, z), dim=1).to(torch.int32)


def key_batch(keys):
    """int64 keys -> their batch index (int64)."""
    return keys >> 48


def scene_floor_keys(nseg, device):
    """[nseg + 1] int64: the smallest key of each scene 0 .. nseg; scene s of a sorted key vector lies between the lower bounds
    of entries s and s + 1."""
    return torch.arange(nseg + 1, dtype=torch.int64, device=device) << 48


def origin_keys(num_scenes, device):
    """[num_scenes] int64: the key of the site (b, 0, 0, 0) of every scene, in order."""
    centre = (KEY_BIAS << 32) | (KEY_BIAS << 16) | KEY_BIAS
    return (torch.arange(num_scenes, dtype=torch.int64, device=device) << 48) | centre


def kernel_map(in_keys, out_keys, offsets):
    """nbr [K, Nout] int32: row of the (sorted) input site at out_keys[u] + offsets[k], -1 where unoccupied."""
    L.require_gpu(in_keys, "in_keys")
    assert in_keys.dtype == torch.int64 and out_keys.dtype == torch.int64 and offsets.dtype == torch.int32
    K, nout = offsets.shape[0], out_keys.shape[0]
    nbr = torch.empty((K, nout), dtype=torch.int32, device=in_keys.device)
    L.check(L.lib().vdetr_sp_kernel_map_i32(L.ptr(in_keys.contiguous()), in_keys.shape[0], L.ptr(out_keys.contiguous()), nout,
                                            L.ptr(offsets.contiguous()), K, L.ptr(nbr), L.stream_ptr()), "sp_kernel_map")
    return nbr


def inverse_map(nbr, nin):
    """inv [K, Nin] int32: the output row that reads input row i through offset k (unique on a lattice), -1 if none."""
    L.require_gpu(nbr, "nbr")
    K, nout = nbr.shape
    inv = torch.full((K, nin), -1, dtype=torch.int32, device=nbr.device)
    L.check(L.lib().vdetr_sp_inverse_map_i32(L.ptr(nbr), K, nout, nin, L.ptr(inv), L.stream_ptr()), "sp_inverse_map")
    return inv


def gather_cols(feats, nbr):
    """col [Nout, K, C] = feats[nbr[k, u]] (zeros where -1); C % 4 == 0."""
    L.require_gpu(feats, "feats")
    L.require_float(feats, "feats")
    L.require_contiguous(feats, "feats")
    K, nout = nbr.shape
    C = feats.shape[1]
    col = torch.empty((nout, K, C), dtype=torch.float32, device=feats.device)
    L.check(L.lib().vdetr_sp_gather_cols_f32(L.ptr(feats), L.ptr(nbr), K, nout, C, L.ptr(col), L.stream_ptr()), "sp_gather_cols")
    return col


def gather_sum(dcol, inv, offset_major=False, flat=False):
    """din [Nin, C] = sum_k dcol[inv[k, i], k] (the adjoint of ``gather_cols``, as a gather).  ``offset_major``: dcol is
    [K, M, C] (slice k holds the compacted rows of offset k) instead of [Nout, K, C]; ``flat``: dcol is [P, C] and ``inv``
    holds absolute rows (the pair lists of PairPlan)."""
    L.require_gpu(dcol, "dcol")
    L.require_float(dcol, "dcol")
    L.require_contiguous(dcol, "dcol")
    K, nin = inv.shape
    C = dcol.shape[-1]
    M = -1 if flat else (dcol.shape[1] if offset_major else 0)
    assert flat or dcol.shape[0 if offset_major else 1] == K
    din = torch.empty((nin, C), dtype=torch.float32, device=dcol.device)
    L.check(L.lib().vdetr_sp_gather_sum_f32(L.ptr(dcol), L.ptr(inv), K, nin, C, M, L.ptr(din), L.stream_ptr()), "sp_gather_sum")
    return din


class _SparseConvFn(Function):
    """out [Nout, Cout] = sum_k feats[nbr[k]] @ W[k]   (W [K, Cin, Cout]); gradients w.r.t. feats and W."""

    @staticmethod
    def forward(ctx, feats, weight, nbr, inv):
        K, cin, cout = weight.shape
        col = gather_cols(feats, nbr)                       # [Nout, K, Cin]
        out = col.view(col.shape[0], K * cin) @ weight.reshape(K * cin, cout)
        ctx.save_for_backward(col, weight, inv)
        return out

    @staticmethod
    def backward(ctx, dout):
        col, weight, inv = ctx.saved_tensors
        K, cin, cout = weight.shape
        dout = dout.contiguous()
        dw = dfeats = None
        if ctx.needs_input_grad[1]:
            dw = (col.view(col.shape[0], K * cin).t() @ dout).view(K, cin, cout)
        if ctx.needs_input_grad[0]:
            dcol = (dout @ weight.reshape(K * cin, cout).t()).view(-1, K, cin)
            dfeats = gather_sum(dcol, inv)
        return dfeats, dw, None, None


class ConvPlan:
    """Geometry of one sparse convolution, compacted per kernel offset (built once per scene and layer shape, no gradients).

    On indoor scans a site has 3-7 of its 27 neighbours, so the im2col operand of ``_SparseConvFn`` is ~85 % zeros.  The
    plan keeps, for every kernel offset k, only the n_k (output, input) pairs that exist; offsets with similar n_k form a
    GROUP whose lists are padded to the group's longest (M) so that a group is ONE batched GEMM  [Kg, M, Cin] x [Kg, Cin, Cout]:
      src  [Kg, M]    input row of pair j of offset k        (-1 padding)
      rows [Kg, M]    output row of that pair
      slot [Kg, Nout] pair index j of output u in offset k   (-1: u has no neighbour through k)
      islot[Kg, Nin]  pair index j of input i in offset k
    forward  out[u]  = sum_k (A[k] W[k])[slot[k][u]]   with A[k][j] = in[src[k][j]]       (gather, bmm, gather-sum)
    backward din[i]  = sum_k (dP[k] W[k]^T)[islot[k][i]], dW[k] = A[k]^T dP[k], dP[k][j] = dout[rows[k][j]].
    Both reductions are gathers in a fixed order: deterministic, no atomics.  The centre offset of a stride-1 layer is the
    identity map: no gather at all."""

    SORTED_MIN_CHANNELS = 128 * 128  # Cin * Cout from which gathering a group's weights costs less than its padding
    SORTED_SPLIT = 1.3               # hit counts within a count-sorted group differ by at most this factor
    SORTED_MAX_GROUPS = 6

    def __init__(self, nbr, nin):
        K, nout = nbr.shape
        self.nin, self.nout, self.K = nin, nout, K
        self.nbr = nbr
        self.counts = (nbr >= 0).sum(1).tolist()  # geometry phase: one sync per plan
        self.pairs = int(sum(self.counts))
        self.ident = None  # the centre offset of a stride-1 layer maps every site to itself: a plain GEMM, no gather
        if nin == nout and K % 2 == 1 and self.counts[K // 2] == nout:
            if bool((nbr[K // 2] == torch.arange(nin, dtype=torch.int32, device=nbr.device)).all()):
                self.ident = K // 2
        self._groups = {}
        self.groups = self.grouping("ranges")
        self.padded_pairs = sum(g["n"] * g["M"] for g in self.groups)

    def grouping(self, kind):
        """"ranges": groups are CONTIGUOUS offset ranges, a group's weights are the view W[k0:k1] (no copy of the parameter,
        no scatter of its gradient) — the identity offset on its own, the ranges before / after it as one batched GEMM each.
        "sorted": offsets sorted by hit count and cut wherever the count drops by SORTED_SPLIT: ~1.15x padding instead of
        ~1.6x, at the price of an index_select of W per group (worth it for wide layers)."""
        if kind not in self._groups:
            K, counts, ident = self.K, self.counts, self.ident
            sets = []
            if kind == "ranges":
                for k0, k1 in ([(0, K)] if ident is None else [(0, ident), (ident + 1, K)]):
                    ks = [k for k in range(k0, k1)]
                    if ks and max(counts[k] for k in ks) > 0:
                        sets.append(ks)
            else:
                order = sorted((k for k in range(K) if counts[k] > 0 and k != ident), key=lambda k: -counts[k])
                while order:
                    top = counts[order[0]]
                    ks = [k for k in order if counts[k] * self.SORTED_SPLIT >= top] if len(sets) < self.SORTED_MAX_GROUPS - 1 else order
                    order = [k for k in order if k not in ks]
                    sets.append(sorted(ks))
            groups = [self._build(ks) for ks in sets]
            if ident is not None:
                groups.insert(1 if kind == "ranges" and len(groups) > 1 else 0,
                              {"ks": [ident], "k0": ident, "k1": ident + 1, "n": 1, "identity": True, "M": self.nout})
            self._groups[kind] = groups
        return self._groups[kind]

    def _build(self, ks):
        nbr, dev = self.nbr, self.nbr.device
        contiguous = ks == list(range(ks[0], ks[-1] + 1))
        sel = nbr[ks[0]:ks[-1] + 1] if contiguous else nbr[torch.tensor(ks, dtype=torch.int64, device=dev)]
        M = max(self.counts[k] for k in ks)
        v = sel >= 0
        slot = torch.where(v, v.cumsum(1, dtype=torch.int32) - 1, torch.full_like(sel, -1))
        kloc, u = torch.nonzero(v, as_tuple=True)
        j = slot[kloc, u].long()
        i = sel[kloc, u]
        rows = torch.full((len(ks), M), -1, dtype=torch.int32, device=dev)
        src = torch.full((len(ks), M), -1, dtype=torch.int32, device=dev)
        islot = torch.full((len(ks), self.nin), -1, dtype=torch.int32, device=dev)
        rows[kloc, j] = u.int()
        src[kloc, j] = i
        islot[kloc, i.long()] = j.int()
        return {"ks": ks, "k0": ks[0] if contiguous else None, "k1": ks[-1] + 1 if contiguous else None, "n": len(ks),
                "kidx": None if contiguous else torch.tensor(ks, dtype=torch.int64, device=dev), "identity": False, "M": M,
                "src": src, "rows": rows, "slot": slot.contiguous(), "islot": islot}

    def select(self, cin, cout):
        return self.grouping("sorted" if cin * cout >= self.SORTED_MIN_CHANNELS else "ranges")


def _group_weight(weight, g):
    return weight[g["k0"]:g["k1"]] if g["k0"] is not None else weight.index_select(0, g["kidx"])


class _PlannedConvFn(Function):
    """out [Nout, Cout] = sum_k in[nbr[k]] @ W[k] through a ConvPlan (see there)."""

    @staticmethod
    def forward(ctx, feats, weight, plan):
        groups = plan.select(weight.shape[1], weight.shape[2])
        out, saved = None, []
        for g in groups:
            w = _group_weight(weight, g)
            if g["identity"]:
                part, a3 = feats @ w[0], feats
            else:
                kg, M = g["src"].shape
                a3 = gather_cols(feats, g["src"].view(1, kg * M)).view(kg, M, feats.shape[1])
                part = gather_sum(torch.bmm(a3, w), g["slot"], offset_major=True)
            saved.append(a3)
            out = part if out is None else out.add_(part)
        if out is None:
            out = feats.new_zeros((plan.nout, weight.shape[2]))
        ctx.plan, ctx.groups = plan, groups
        ctx.save_for_backward(weight, *saved)
        return out

    @staticmethod
    def backward(ctx, dout):
        weight, *saved = ctx.saved_tensors
        plan = ctx.plan
        dout = dout.contiguous()
        need_f, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dfeats = None
        dw = torch.zeros_like(weight) if need_w else None
        for g, a3 in zip(ctx.groups, saved):
            w = _group_weight(weight, g)
            if g["identity"]:
                if need_w:
                    torch.mm(a3.t(), dout, out=dw[g["k0"]])
                part = dout @ w[0].t() if need_f else None
            else:
                kg, M = g["rows"].shape
                dp = gather_cols(dout, g["rows"].view(1, kg * M)).view(kg, M, dout.shape[1])
                if need_w:
                    if g["k0"] is not None:
                        torch.bmm(a3.transpose(1, 2), dp, out=dw[g["k0"]:g["k1"]])
                    else:
                        dw.index_copy_(0, g["kidx"], torch.bmm(a3.transpose(1, 2), dp))
                part = gather_sum(torch.bmm(dp, w.transpose(1, 2)), g["islot"], offset_major=True) if need_f else None
            if need_f:
                dfeats = part if dfeats is None else dfeats.add_(part)
        if need_f and dfeats is None:
            dfeats = dout.new_zeros((plan.nin, weight.shape[1]))
        return dfeats, dw, None


class _PinnedCounts:
    """a ring of pinned host rows for the asynchronous copies of the plans' pair counts (one allocation per process)"""
    rows, width = 512, 64
    _buf, _next = None, 0
    _lock = threading.Lock()

    @classmethod
    def take(cls, n):
        assert n <= cls.width
        with cls._lock:
            if cls._buf is None:
                cls._buf = torch.empty((cls.rows, cls.width), dtype=torch.int32, pin_memory=True)
            row = cls._buf[cls._next % cls.rows]
            cls._next += 1
        return row[:n]


class PairPlan:
    """Geometry of one sparse convolution as a PAIR LIST sorted by kernel offset (built once per scene and layer shape):
      pin [P], pout [P]   input / output row of pair p; the pairs of offset k are the segment seg[k] .. seg[k+1]
      slot [K, Nout]      pair (absolute index) through which output u reads offset k, -1 if none
      islot [K, Nin]      pair through which input i is read with offset k
      tiles [T, 3]        (k, first pair, count <= 128): the 128-pair tiles of vdetr_sp_pairs_gemm_f32
    Nothing is padded: the fused kernels (csrc/sparse_conv.hip) gather rows straight into the matrix-core operands.

    On the GPU the lists are built by vdetr_sp_pair_plan_i32 without a host round trip; what needs the pair COUNTS on the host
    (P, seg, tiles, the weight-gradient chunks) is derived on first use from an asynchronous copy, so that a whole scene's
    plans cost one synchronisation instead of three each."""

    _LAZY = ("P", "pairs", "counts", "seg", "tiles", "ntiles", "pin", "pout")
    WGRAD_WORKGROUPS = 768  # workgroups per weight-gradient launch: ~3 per CU

    def __init__(self, nbr, nin):
        K, nout = nbr.shape
        self.K, self.nin, self.nout = K, nin, nout
        self._chunks = {}
        self._pending = None
        if nbr.is_cuda and K + 1 <= _PinnedCounts.width:
            self._launch(nbr)
        else:
            self._build_host(nbr)

    # ---- tensor-expression construction (CPU tensors: the host statement the device builder is tested against) --------
    def _build_host(self, nbr):
        K, nout, nin, dev = self.K, self.nout, self.nin, nbr.device
        valid = nbr >= 0
        counts = valid.sum(1).tolist()
        pk, pout = torch.nonzero(valid, as_tuple=True)      # sorted by (k, u)
        P = int(pk.shape[0])
        self.pout = pout.int().contiguous()
        self.pin = nbr[pk, pout].contiguous()
        idx = torch.arange(P, dtype=torch.int32, device=dev)
        self.slot = torch.full((K, nout), -1, dtype=torch.int32, device=dev)
        self.slot[pk, pout] = idx
        self.islot = torch.full((K, nin), -1, dtype=torch.int32, device=dev)
        self.islot[pk, self.pin.long()] = idx
        self._tables(counts)

    # ---- device construction ------------------------------------------------------------------------------------------
    def _launch(self, nbr):
        K, nout, nin, dev = self.K, self.nout, self.nin, nbr.device
        lib = L.lib()
        nbr = nbr.contiguous()
        cap = max(K * nout, 1)
        self._pin_buf = torch.empty(cap, dtype=torch.int32, device=dev)
        self._pout_buf = torch.empty(cap, dtype=torch.int32, device=dev)
        self.slot = torch.empty((K, nout), dtype=torch.int32, device=dev)
        self.islot = torch.empty((K, nin), dtype=torch.int32, device=dev)
        counts_dev = torch.empty(K + 1, dtype=torch.int32, device=dev)
        ws = L.workspace(4 * max(lib.vdetr_sp_pair_plan_workspace_ints(K, nout), 1), dev).view(torch.int32)
        L.check(lib.vdetr_sp_pair_plan_i32(L.ptr(nbr), K, nout, nin, L.ptr(self._pin_buf), L.ptr(self._pout_buf), L.ptr(self.slot),
                                           L.ptr(self.islot) if nin else None, L.ptr(counts_dev), L.ptr(ws), L.stream_ptr()),
                "sp_pair_plan")
        host = _PinnedCounts.take(K + 1)
        host.copy_(counts_dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending = (host, ev, counts_dev, ws)  # device buffers kept alive until the copy has landed

    def finalize(self):
        """wait for the pair counts (no-op once done) and derive the host-side tables"""
        if self._pending is not None:
            host, ev, _, _ = self._pending
            ev.synchronize()
            counts = host.tolist()
            self._pending = None
            P = counts[self.K]
            self.pin, self.pout = self._pin_buf[:P], self._pout_buf[:P]
            self._tables(counts[:self.K])
            for cin, cout in sorted(self.__dict__.pop("_wanted", ())):
                self.wgrad_chunks(cin, cout)
        return self

    def __getattr__(self, name):  # only reached for attributes not set yet
        if name in PairPlan._LAZY and self.__dict__.get("_pending") is not None:
            self.finalize()
            return self.__dict__[name]
        raise AttributeError(name)

    @staticmethod
    def _cut(counts, seg, L):
        """every segment k (seg[k], counts[k]) cut into pieces of at most L: (k, start, length) arrays and pieces per segment;
        array arithmetic instead of a Python loop per piece (a scene has ~10^4 pieces over its 16 plans, and the loader thread
        that builds them shares the interpreter lock with the thread that launches the training step)"""
        counts = np.asarray(counts, dtype=np.int64)
        per = -(-counts // L)
        kidx = np.repeat(np.arange(counts.shape[0], dtype=np.int64), per)
        first = np.cumsum(per) - per
        within = np.arange(kidx.shape[0], dtype=np.int64) - first[kidx]
        start = np.asarray(seg[:-1], dtype=np.int64)[kidx] + within * L
        length = np.minimum(L, counts[kidx] - within * L)
        return kidx, start, length, per

    def _tables(self, counts):
        dev = self.slot.device
        self.counts = counts
        self.P = self.pairs = int(sum(counts))
        seg = [0]
        for c in counts:
            seg.append(seg[-1] + c)
        self.seg = seg
        kidx, start, length, _ = PairPlan._cut(counts, seg, 128)
        self.ntiles = int(kidx.shape[0])
        tiles = np.stack([kidx, start, length], 1).astype(np.int32) if self.ntiles else np.zeros((1, 3), np.int32)
        self.tiles = torch.from_numpy(tiles).to(dev)

    def request_wgrad(self, cin, cout):
        """a layer of cin x cout channels will ask for wgrad_chunks: build that table with the geometry (`finalize`), not inside
        the backward pass, where its upload would make the launching thread wait for the device"""
        cin, cout = cin + (-cin) % 16, cout + (-cout) % 16  # (sparse_conv pads the channels of the fused kernels to 16)
        if self.__dict__.get("_pending") is None:
            self.wgrad_chunks(cin, cout)
        else:
            self.__dict__.setdefault("_wanted", set()).add((cin, cout))

    def wgrad_chunks(self, cin, cout):
        """(chunks [n, 4] i32, cseg [K+1] i32, n): every offset's segment cut into chunks of at most L pairs, L chosen so that
        the launch has ~3 workgroups per CU.  Chunks of EQUAL length, not an equal number of chunks per offset: the centre
        offset holds a quarter of all pairs, and a launch is as slow as its longest workgroup.  Chunk c writes partial c;
        the partials of offset k are cseg[k] .. cseg[k+1]."""
        t = 128 if (cin >= 128 and cout >= 128) else 64  # channel tile of vdetr_sp_pairs_wgrad_f32
        key = (-(-cin // t)) * (-(-cout // t))
        if key not in self._chunks:
            want = max(1, self.WGRAD_WORKGROUPS // key)
            L = max(64, -(-(-(-self.P // want)) // 16) * 16)
            kidx, start, length, per = PairPlan._cut(self.counts, self.seg, L)
            n = int(kidx.shape[0])
            rows = np.stack([kidx, start, length, np.arange(n, dtype=np.int64)], 1).astype(np.int32) if n else np.zeros((1, 4), np.int32)
            cseg = np.concatenate([[0], np.cumsum(per)]).astype(np.int32)
            dev = self.slot.device
            self._chunks[key] = (torch.from_numpy(rows).to(dev), torch.from_numpy(cseg).to(dev), n)
        return self._chunks[key]


def pairs_gemm(x, arow, weight, plan, transposed):
    """y [P, Cout] = x[arow[p]] @ W[k(p)]  (transposed: y [P, Cin] = x[arow[p]] @ W[k(p)]^T)"""
    L.require_gpu(x, "x")
    L.require_float(x, "x")
    L.require_contiguous(x, "x")
    K, cin, cout = weight.shape
    if x.numel() * 4 >= 2 ** 32 or cin * cout * 4 >= 2 ** 32:
        raise RuntimeError("pairs_gemm: a feature table of 4 GB or more (32-bit buffer offsets in the persistent kernel): split the batch")
    y = torch.empty((plan.P, cin if transposed else cout), dtype=torch.float32, device=x.device)
    L.check(L.lib().vdetr_sp_pairs_gemm_f32(L.ptr(x), L.ptr(arow), L.ptr(weight), L.ptr(plan.tiles), plan.ntiles, cin, cout,
                                            1 if transposed else 0, L.ptr(y), L.stream_ptr()), "sp_pairs_gemm")
    return y


def pairs_wgrad(x, dy, plan, cin, cout):
    """dW [K, Cin, Cout] = sum over the pairs of offset k of x[pin[p]]^T dy[pout[p]]"""
    L.require_gpu(x, "x")
    L.require_contiguous(x, "x")
    L.require_contiguous(dy, "dy")
    chunks, cseg, n = plan.wgrad_chunks(cin, cout)
    part = torch.empty((max(n, 1), cin, cout), dtype=torch.float32, device=x.device)
    L.check(L.lib().vdetr_sp_pairs_wgrad_f32(L.ptr(x), L.ptr(dy), L.ptr(plan.pin), L.ptr(plan.pout), L.ptr(chunks),
                                             n, cin, cout, L.ptr(part), L.stream_ptr()), "sp_pairs_wgrad")
    dw = torch.empty((plan.K, cin, cout), dtype=torch.float32, device=x.device)
    L.check(L.lib().vdetr_sp_wgrad_reduce_f32(L.ptr(part), L.ptr(cseg), plan.K, cin * cout, L.ptr(dw), L.stream_ptr()),
            "sp_wgrad_reduce")
    return dw


class _PairsConvFn(Function):
    """out [Nout, Cout] = sum_k in[nbr[k]] @ W[k] through a PairPlan and the fused matrix-core kernels."""

    @staticmethod
    def forward(ctx, feats, weight, plan):
        weight = weight.contiguous()
        if plan.P == 0:  # no site of the layer has a neighbour (a 1x1x1 stride-2 layer on a tiny cloud)
            out = feats.new_zeros((plan.nout, weight.shape[2]))
        else:
            out = gather_sum(pairs_gemm(feats, plan.pin, weight, plan, False), plan.slot, flat=True)
        ctx.plan = plan
        ctx.save_for_backward(feats, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        feats, weight = ctx.saved_tensors
        plan = ctx.plan
        dout = dout.contiguous()
        K, cin, cout = weight.shape
        dfeats = dw = None
        if plan.P == 0:
            return (feats.new_zeros(feats.shape) if ctx.needs_input_grad[0] else None,
                    torch.zeros_like(weight) if ctx.needs_input_grad[1] else None, None)
        if ctx.needs_input_grad[0]:
            dfeats = gather_sum(pairs_gemm(dout, plan.pout, weight, plan, True), plan.islot, flat=True)
        if ctx.needs_input_grad[1]:
            dw = pairs_wgrad(feats, dout, plan, cin, cout)
        return dfeats, dw, None


_ACT = {None: 0, "none": 0, "relu": 1, "elu": 2}


class _SpBnActFn(Function):
    """y = act(batch_norm(x) + residual) over a point-major table [N, C] (csrc/sp_bn.hip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, nbt, training, momentum, eps, act):
        L.require_gpu(x, "x")
        L.require_float(x, "x")
        x = x.contiguous()
        N, C = x.shape
        lib = L.lib()
        d = L.SpBnDesc()
        d.N, d.C, d.act, d.training, d.eps, d.momentum = N, C, act, 1 if training else 0, float(eps), float(momentum)
        y = torch.empty_like(x)
        save_mean = torch.empty(C, dtype=torch.float32, device=x.device)
        save_invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = L.workspace(lib.vdetr_sp_bn_workspace_bytes(N, C), x.device)
        res = residual.contiguous() if residual is not None else None
        d.x, d.gamma, d.beta, d.residual = x.data_ptr(), L.ptr(gamma).value, L.ptr(beta).value, L.ptr(res).value
        d.running_mean, d.running_var = L.ptr(running_mean).value, L.ptr(running_var).value
        d.num_batches_tracked = L.ptr(nbt).value if training else None
        d.y, d.save_mean, d.save_invstd, d.workspace = y.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(), ws.data_ptr()
        L.check(lib.vdetr_sp_bn_act_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_bn_act_fwd")
        ctx.save_for_backward(x, gamma, y, save_mean, save_invstd)
        ctx.cfg = (act, training, eps, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, y, save_mean, save_invstd = ctx.saved_tensors
        act, training, eps, has_res = ctx.cfg
        N, C = x.shape
        lib = L.lib()
        dy = dy.contiguous()
        d = L.SpBnDesc()
        d.N, d.C, d.act, d.training, d.eps = N, C, act, 1 if training else 0, float(eps)
        ws = L.workspace(lib.vdetr_sp_bn_workspace_bytes(N, C), x.device)
        d.x, d.gamma, d.y = x.data_ptr(), L.ptr(gamma).value, y.data_ptr()
        d.save_mean, d.save_invstd, d.workspace = save_mean.data_ptr(), save_invstd.data_ptr(), ws.data_ptr()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dres = torch.empty_like(x) if (has_res and ctx.needs_input_grad[3]) else None
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device) if gamma is not None else None
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device) if gamma is not None else None
        L.check(lib.vdetr_sp_bn_act_bwd_f32(ctypes.byref(d), L.ptr(dy), L.ptr(dx), L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta),
                                            L.stream_ptr()), "sp_bn_act_bwd")
        return dx, dgamma, dbeta, dres, None, None, None, None, None, None, None


class _SpSyncBnActFn(Function):
    """_SpBnActFn with batch statistics over all data-parallel ranks (bn_act.set_sync; the reference converts the backbone's
    BatchNorms to SyncBatchNorm like every other, main.py:512-514).  Ranks hold different site counts: the local (mean, M2,
    N) triples are all-gathered and merged; the normalisation itself is the fused launch (its running-statistics path, fed
    with the global batch statistics); the backward's two sums are all-reduced between its reduction and its element pass,
    which therefore run as tensor expressions here."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, nbt, momentum, eps, act):
        import torch.distributed as dist
        from . import bn_act as BNA
        x = x.contiguous()
        N, C = x.shape
        grp = BNA._sync["group"]
        var_l, mean_l = torch.var_mean(x, 0, unbiased=False)
        loc = torch.stack((mean_l, var_l * N, torch.full_like(mean_l, float(N))))
        world = dist.get_world_size(grp)
        allr = torch.empty((world, 3, C), dtype=torch.float32, device=x.device)
        dist.all_gather(list(allr.unbind(0)), loc, group=grp)
        cnt = allr[:, 2]
        n = cnt.sum(0)
        mean = (allr[:, 0] * cnt).sum(0) / n
        m2 = (allr[:, 1] + cnt * (allr[:, 0] - mean) ** 2).sum(0)
        var = m2 / n
        if running_mean is not None:
            running_mean.mul_(1.0 - momentum).add_(mean, alpha=momentum)
            running_var.mul_(1.0 - momentum).add_(m2 / torch.clamp(n - 1.0, min=1.0), alpha=momentum)
        if nbt is not None:
            nbt += 1
        lib = L.lib()
        d = L.SpBnDesc()
        d.N, d.C, d.act, d.training, d.eps, d.momentum = N, C, act, 0, float(eps), float(momentum)
        y = torch.empty_like(x)
        res = residual.contiguous() if residual is not None else None
        mean_c, var_c = mean.contiguous(), var.contiguous()
        d.x, d.gamma, d.beta, d.residual = x.data_ptr(), L.ptr(gamma).value, L.ptr(beta).value, L.ptr(res).value
        d.running_mean, d.running_var, d.y = mean_c.data_ptr(), var_c.data_ptr(), y.data_ptr()
        L.check(lib.vdetr_sp_bn_act_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_bn_act_fwd")
        invstd = torch.rsqrt(var + eps)
        ctx.save_for_backward(x, gamma, y, mean_c, invstd, (1.0 / n[:1]))
        ctx.cfg = (act, residual is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        import torch.distributed as dist
        from . import bn_act as BNA
        x, gamma, y, mean, invstd, inv_n = ctx.saved_tensors
        act, has_res = ctx.cfg
        g = dy
        if act == 1:
            g = dy * (y > 0)
        elif act == 2:
            g = dy * torch.where(y > 0, torch.ones_like(y), y + 1.0)
        xhat = (x - mean) * invstd
        loc = torch.stack((g.sum(0), (g * xhat).sum(0)))
        tot = loc.clone()
        dist.all_reduce(tot, group=BNA._sync["group"])
        k = invstd if gamma is None else gamma * invstd
        dx = k * (g - tot[0] * inv_n - xhat * (tot[1] * inv_n)) if ctx.needs_input_grad[0] else None
        return dx, (loc[1] if gamma is not None else None), (loc[0] if gamma is not None else None), \
            (g if has_res and ctx.needs_input_grad[3] else None), None, None, None, None, None, None


def bn_act(x, bn, act=None, residual=None):
    """act(bn(x) + residual) for an ``nn.BatchNorm1d`` module over the rows of x [N, C]: one fused HIP pass on the GPU; any
    other module type (SyncBatchNorm) or a CPU tensor goes through the module itself and plain torch ops."""
    # (sp_bn.hip holds one float4 of a row per thread, 256 threads: up to 1024 channels; momentum=None is a cumulative
    # average, which the kernels do not do: both go through the module)
    fused = x.is_cuda and type(bn) is torch.nn.BatchNorm1d and x.shape[1] % 4 == 0 and 0 < x.shape[1] <= 1024 and x.shape[0] > 0 \
        and (bn.momentum is not None or not bn.training)
    if not fused:
        from . import bn_act as BNA
        # (with bn_act.set_sync this is still a cross-replica BatchNorm — as tensor expressions — and a rank whose tensor is
        # EMPTY joins its collectives with a count of zero instead of leaving the other ranks waiting)
        y = BNA.batch_norm_module(bn, x, channel_last=True)
        if residual is not None:
            y = y + residual
        return torch.relu(y) if act == "relu" else torch.nn.functional.elu(y) if act == "elu" else y
    training = bn.training or bn.running_mean is None
    momentum = 0.1 if bn.momentum is None else bn.momentum
    if training:
        from . import bn_act as BNA
        if BNA.sync_active():
            return _SpSyncBnActFn.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var,
                                        bn.num_batches_tracked if bn.track_running_stats else None, momentum, bn.eps, _ACT[act])
    return _SpBnActFn.apply(x, bn.weight, bn.bias, residual, bn.running_mean, bn.running_var,
                            bn.num_batches_tracked if bn.track_running_stats else None, training, momentum, bn.eps, _ACT[act])


def _pair_operands(feats, weight):
    """the operands of the fused pair kernels: they contract over multiples of 16 channels on either side (forward: Cin, input
    gradient: Cout), so both widths are zero-padded to 16"""
    pi, po = (-feats.shape[1]) % 16, (-weight.shape[2]) % 16
    if pi or po:
        feats = torch.nn.functional.pad(feats, (0, pi))
        weight = torch.nn.functional.pad(weight, (0, po, 0, pi))
    return feats.contiguous(), weight


def pair_products(feats, weight, plan):
    """The pair path of ``sparse_conv`` up to its gather-sum, for an inference caller that finishes the rows itself
    (``gather_sum_bn_act``): y [P, Cout padded to 16] = feats[pin[p]] @ W[k(p)], or None when the layer has no pair at all.
    ``gather_sum(y, plan.slot, flat=True)[:, :Cout]`` is what ``sparse_conv`` returns.  No autograd."""
    feats, weight = _pair_operands(feats, weight)
    return pairs_gemm(feats, plan.pin, weight.contiguous(), plan, False) if plan.P else None


def gather_sum_bn_act(y, slot, bn, act=None, residual=None, post_add=None, conv_bias=None, channels=None):
    """act(bn(gather_sum(y, slot)[:, :channels] + conv_bias) + residual) + post_add in ONE launch, for an ``nn.BatchNorm1d``
    with running statistics (eval mode; vdetr_sp_gather_sum_bn_act_f32).  y [P, stride >= channels] are a layer's pair products
    (``pair_products``; None: the layer has no pair), slot [K, N] its PairPlan.slot; residual / post_add [N, channels],
    conv_bias [channels] or [1, channels].  Reads bn's own tensors at every call: nothing is cached.  No autograd."""
    L.require_gpu(slot, "slot")
    L.require_int(slot, "slot")
    L.require_contiguous(slot, "slot")
    K, n = slot.shape
    d = L.SpGsumBnDesc()
    if y is not None:
        L.require_gpu(y, "y")
        L.require_float(y, "y")
        L.require_contiguous(y, "y")
        d.src, d.src_stride = y.data_ptr(), y.shape[1]
    C = channels if channels is not None else (y.shape[1] if y is not None else bn.num_features)
    if y is None:
        d.src_stride = C
    if bn.running_mean is None or bn.running_var is None or bn.num_features != C:
        raise RuntimeError(f"gather_sum_bn_act: a BatchNorm1d of {C} channels with running statistics is required")
    out = torch.empty((n, C), dtype=torch.float32, device=slot.device)
    d.K, d.nrows, d.C, d.act, d.eps = K, n, C, _ACT[act], float(bn.eps)
    keep = []  # (the contiguous copies the descriptor points into)
    for name, t, numel in (("conv_bias", conv_bias, C), ("gamma", bn.weight, C), ("beta", bn.bias, C), ("running_mean", bn.running_mean, C),
                           ("running_var", bn.running_var, C), ("residual", residual, n * C), ("post_add", post_add, n * C)):
        if t is None:
            continue
        L.require_gpu(t, name)
        L.require_float(t, name)
        if t.numel() != numel:
            raise RuntimeError(f"gather_sum_bn_act: {name} has {t.numel()} elements, expected {numel}")
        t = t.detach().contiguous()
        keep.append(t)
        setattr(d, name, t.data_ptr())
    d.slot, d.out = slot.data_ptr(), out.data_ptr()
    L.check(L.lib().vdetr_sp_gather_sum_bn_act_f32(ctypes.byref(d), L.stream_ptr()), "sp_gather_sum_bn_act")
    return out


POOL_MODES = {"sum": L.VDETR_POOL_SUM, "avg": L.VDETR_POOL_AVG, "max": L.VDETR_POOL_MAX}


class _SparsePoolFn(Function):
    """y [Nout, C] = sum / average / maximum of feats[nbr[k, u]] over the neighbours that exist (csrc/sparse_pool.hip)."""

    @staticmethod
    def forward(ctx, feats, nbr, inv, mode):
        K, nout = nbr.shape
        nin, C = feats.shape
        dev = feats.device
        d = L.SpPoolDesc()
        d.K, d.nout, d.nin, d.C, d.mode = K, nout, nin, C, mode
        y = torch.empty((nout, C), dtype=torch.float32, device=dev)
        inv_count = torch.empty(nout, dtype=torch.float32, device=dev) if mode == L.VDETR_POOL_AVG else None
        arg = torch.empty((nout, C), dtype=torch.int8, device=dev) if mode == L.VDETR_POOL_MAX else None
        d.x, d.nbr, d.y = feats.data_ptr(), nbr.data_ptr(), y.data_ptr()
        d.inv_count, d.arg = L.ptr(inv_count).value, L.ptr(arg).value
        L.check(L.lib().vdetr_sp_pool_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_pool_fwd")
        ctx.save_for_backward(inv, inv_count, arg)
        ctx.cfg = (K, nout, nin, C, mode)
        ctx.mark_non_differentiable(*(t for t in (inv_count, arg) if t is not None))
        return y, inv_count, arg

    @staticmethod
    def backward(ctx, dy, _dcount, _darg):
        inv, inv_count, arg = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return _sparse_pool_backward(dy.contiguous(), inv, ctx.cfg, inv_count, arg), None, None, None


def _sparse_pool_backward(dy, inv, cfg, inv_count, arg):
    """the backward launch of ``_SparsePoolFn`` (cfg = (K, nout, nin, C, mode)): dx [Nin, C]"""
    K, nout, nin, C, mode = cfg
    d = L.SpPoolDesc()
    d.K, d.nout, d.nin, d.C, d.mode = K, nout, nin, C, mode
    d.inv_count, d.arg = L.ptr(inv_count).value, L.ptr(arg).value
    dx = torch.empty((nin, C), dtype=torch.float32, device=dy.device)
    L.check(L.lib().vdetr_sp_pool_bwd_f32(ctypes.byref(d), L.ptr(inv), L.ptr(dy), L.ptr(dx), L.stream_ptr()), "sp_pool_bwd")
    return dx


def sparse_pool(feats, nbr, inv, mode, return_aux=False):
    """Pooling over a kernel map: feats [Nin, C] (contiguous fp32 on the device, C % 4 == 0), nbr [K, Nout] (``kernel_map``),
    inv [K, Nin] (``inverse_map(nbr, Nin)``; None: built here), mode "sum" | "avg" | "max" -> y [Nout, C].  avg divides by the
    neighbours that exist; a site without any gives 0 in every mode and passes no gradient.  One launch forward, one backward (a
    gather through ``inv``): deterministic.  ``return_aux``: also (inv_count [Nout] or None, arg [Nout, C] int8 or None)."""
    L.require_gpu(feats, "feats")
    L.require_float(feats, "feats")
    L.require_contiguous(feats, "feats")
    L.require_gpu(nbr, "nbr")
    L.require_int(nbr, "nbr")
    L.require_contiguous(nbr, "nbr")
    if mode not in POOL_MODES:
        raise ValueError(f"sparse_pool: mode {mode!r} (sum, avg, max)")
    if feats.dim() != 2 or nbr.dim() != 2:
        raise RuntimeError("sparse_pool: feats must be [Nin, C] and nbr [K, Nout]")
    if inv is None:
        inv = inverse_map(nbr, feats.shape[0])
    L.require_gpu(inv, "inv")
    L.require_int(inv, "inv")
    L.require_contiguous(inv, "inv")
    if tuple(inv.shape) != (nbr.shape[0], feats.shape[0]):
        raise RuntimeError(f"sparse_pool: inv is {tuple(inv.shape)}, expected {(nbr.shape[0], feats.shape[0])}")
    y, inv_count, arg = _SparsePoolFn.apply(feats, nbr, inv, POOL_MODES[mode])
    return (y, inv_count, arg) if return_aux else y


def cwconv_chunk_rows(nout):
    """output rows per chunk of the weight-gradient sweep of sparse_cwconv.hip on a table of nout rows"""
    return int(L.lib().vdetr_sp_cwconv_chunk_rows(int(nout)))


def _cwconv_desc(K, nout, nin, C):
    d = L.SpCwConvDesc()
    d.K, d.nout, d.nin, d.C = K, nout, nin, C
    return d


class _ChannelwiseConvFn(Function):
    """y [Nout, C] = (sum_k weight[k] * feats[nbr[k, u]] over the neighbours that exist) + bias (csrc/sparse_cwconv.hip)."""

    @staticmethod
    def forward(ctx, feats, weight, bias, nbr, inv):
        K, nout = nbr.shape
        nin, C = feats.shape
        b = bias.detach().reshape(-1) if bias is not None else None
        y = torch.empty((nout, C), dtype=torch.float32, device=feats.device)
        d = _cwconv_desc(K, nout, nin, C)
        d.x, d.nbr, d.w, d.bias, d.y = feats.data_ptr(), nbr.data_ptr(), weight.data_ptr(), L.ptr(b).value, y.data_ptr()
        L.check(L.lib().vdetr_sp_cwconv_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_cwconv_fwd")
        ctx.save_for_backward(feats, weight, nbr, inv)
        ctx.bias_shape = None if bias is None else bias.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        feats, weight, nbr, inv = ctx.saved_tensors
        K, nout = nbr.shape
        nin, C = feats.shape
        want_x, want_w, want_b = ctx.needs_input_grad[:3]
        want_b = want_b and ctx.bias_shape is not None
        lib, dev = L.lib(), dy.device
        dy = dy.contiguous()
        d = _cwconv_desc(K, nout, nin, C)
        dx = dw = db = None
        if want_x:
            dx = torch.empty((nin, C), dtype=torch.float32, device=dev)
            d.w = weight.data_ptr()
            L.check(lib.vdetr_sp_cwconv_dgrad_f32(ctypes.byref(d), L.ptr(inv), L.ptr(dy), L.ptr(dx), L.stream_ptr()), "sp_cwconv_dgrad")
        if want_w or want_b:
            dw = torch.empty((K, C), dtype=torch.float32, device=dev) if want_w else None
            db = torch.empty(C, dtype=torch.float32, device=dev) if want_b else None
            ws = L.workspace(lib.vdetr_sp_cwconv_workspace_bytes(K, nout, C), dev)
            d.x, d.nbr, d.workspace = feats.data_ptr(), nbr.data_ptr(), ws.data_ptr()
            L.check(lib.vdetr_sp_cwconv_wgrad_f32(ctypes.byref(d), L.ptr(dy), L.ptr(dw), L.ptr(db), L.stream_ptr()), "sp_cwconv_wgrad")
            if db is not None:
                db = db.reshape(ctx.bias_shape)
        return dx, dw, db, None, None


def channelwise_conv(feats, weight, nbr, inv=None, bias=None):
    """Channelwise (depthwise) convolution over a kernel map: feats [Nin, C] (contiguous fp32 on the device, C % 4 == 0,
    4 <= C <= 1024), weight [K, C] (one weight per offset and channel), nbr [K, Nout] (``kernel_map``), inv [K, Nin]
    (``inverse_map(nbr, Nin)``; None: built here when feats needs a gradient), bias [C] or [1, C] or None -> y [Nout, C] =
    (sum_k weight[k] * feats[nbr[k, u]] over the neighbours that exist, one fmaf per term in ascending k) + bias.  A site without
    a neighbour gives the bias (exact +0 without one).  One launch forward; backward one launch for the input gradient (a gather
    through ``inv``) and two for the weight and bias gradients (chunk partials, then a fold), each only when asked for:
    deterministic, no atomics, no host read."""
    op = "channelwise_conv"
    for name, t in (("feats", feats), ("weight", weight), ("bias", bias)):
        if t is not None:
            L.require_gpu(t, name)
            L.require_float(t, name)
            L.require_contiguous(t, name)
    L.require_gpu(nbr, "nbr")
    L.require_int(nbr, "nbr")
    L.require_contiguous(nbr, "nbr")
    if feats.dim() != 2 or nbr.dim() != 2:
        raise RuntimeError(f"{op}: feats must be [Nin, C] (it is {tuple(feats.shape)}) and nbr [K, Nout] (it is {tuple(nbr.shape)})")
    (nin, C), K = feats.shape, nbr.shape[0]
    if C % 4 or not 4 <= C <= 1024:
        raise RuntimeError(f"{op}: C={C} must be a multiple of 4 in 4 .. 1024 (float4 rows)")
    if not 1 <= K <= 127:
        raise RuntimeError(f"{op}: K={K} must be in 1 .. 127")
    if tuple(weight.shape) != (K, C):
        raise RuntimeError(f"{op}: weight is {tuple(weight.shape)}, expected {(K, C)}")
    if bias is not None and tuple(bias.shape) not in ((C,), (1, C)):
        raise RuntimeError(f"{op}: bias is {tuple(bias.shape)}, expected {(C,)} or {(1, C)}")
    if inv is None and feats.requires_grad and torch.is_grad_enabled():
        inv = inverse_map(nbr, nin)
    if inv is not None:
        L.require_gpu(inv, "inv")
        L.require_int(inv, "inv")
        L.require_contiguous(inv, "inv")
        if tuple(inv.shape) != (K, nin):
            raise RuntimeError(f"{op}: inv is {tuple(inv.shape)}, expected {(K, nin)}")
    return _ChannelwiseConvFn.apply(feats, weight, bias, nbr, inv)


class _SpInstanceNormFn(Function):
    """y = (x - mean_s) * rsqrt(var_s + eps) * gamma + beta per scene s = rows seg[s] .. seg[s+1] (csrc/sp_inorm.hip)."""

    @staticmethod
    def forward(ctx, x, seg, nseg, gamma, beta, eps):
        N, C = x.shape
        lib = L.lib()
        d = L.SpInormDesc()
        d.N, d.C, d.nseg, d.eps = N, C, nseg, float(eps)
        y = torch.empty_like(x)
        save_mean = torch.empty((max(nseg, 1), C), dtype=torch.float32, device=x.device)
        save_invstd = torch.empty((max(nseg, 1), C), dtype=torch.float32, device=x.device)
        ws = L.workspace(lib.vdetr_sp_inorm_workspace_bytes(N, C, nseg), x.device)
        g = gamma.detach().reshape(-1).contiguous() if gamma is not None else None
        b = beta.detach().reshape(-1).contiguous() if beta is not None else None
        d.x, d.seg, d.gamma, d.beta = x.data_ptr(), seg.data_ptr(), L.ptr(g).value, L.ptr(b).value
        d.y, d.save_mean, d.save_invstd, d.workspace = y.data_ptr(), save_mean.data_ptr(), save_invstd.data_ptr(), ws.data_ptr()
        L.check(lib.vdetr_sp_inorm_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_inorm_fwd")
        ctx.save_for_backward(x, seg, g, save_mean, save_invstd)
        ctx.cfg = (nseg, float(eps), None if gamma is None else gamma.shape, None if beta is None else beta.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, seg, g, save_mean, save_invstd = ctx.saved_tensors
        nseg, eps, gshape, bshape = ctx.cfg
        N, C = x.shape
        lib = L.lib()
        dy = dy.contiguous()
        d = L.SpInormDesc()
        d.N, d.C, d.nseg, d.eps = N, C, nseg, eps
        ws = L.workspace(lib.vdetr_sp_inorm_workspace_bytes(N, C, nseg), x.device)
        d.x, d.seg, d.gamma = x.data_ptr(), seg.data_ptr(), L.ptr(g).value
        d.save_mean, d.save_invstd, d.workspace = save_mean.data_ptr(), save_invstd.data_ptr(), ws.data_ptr()
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        # (a table without rows launches nothing: its parameter gradients are zeros)
        new = torch.empty if N and nseg else torch.zeros
        dgamma = new(C, dtype=torch.float32, device=x.device) if gshape is not None and ctx.needs_input_grad[3] else None
        dbeta = new(C, dtype=torch.float32, device=x.device) if bshape is not None and ctx.needs_input_grad[4] else None
        L.check(lib.vdetr_sp_inorm_bwd_f32(ctypes.byref(d), L.ptr(dy), L.ptr(dx), L.ptr(dgamma), L.ptr(dbeta), L.stream_ptr()),
                "sp_inorm_bwd")
        return (dx, None, None, dgamma.reshape(gshape) if dgamma is not None else None,
                dbeta.reshape(bshape) if dbeta is not None else None, None)


def scene_segments(keys, nseg):
    """seg [nseg + 1] int32 on the device: scene s of a sorted key vector is the rows seg[s] .. seg[s+1].  No host read."""
    return torch.searchsorted(keys, scene_floor_keys(nseg, keys.device)).to(torch.int32)


def instance_norm(x, seg, nseg, weight=None, bias=None, eps=1e-6):
    """InstanceNorm of a sparse tensor's table x [N, C] (contiguous fp32 on the device, C % 4 == 0, C <= 1024) over the scenes
    ``seg`` [nseg + 1] int32 (``scene_segments``; device): per scene and channel, biased variance.  weight / bias [C] or [1, C].
    Two launches forward, three backward; deterministic; nothing is read back by the host."""
    L.require_gpu(x, "x")
    L.require_float(x, "x")
    L.require_contiguous(x, "x")
    L.require_gpu(seg, "seg")
    L.require_int(seg, "seg")
    L.require_contiguous(seg, "seg")
    if x.dim() != 2 or seg.numel() != nseg + 1:
        raise RuntimeError(f"instance_norm: x must be [N, C] and seg hold nseg + 1 = {nseg + 1} offsets (it holds {seg.numel()})")
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None:
            L.require_gpu(t, name)
            L.require_float(t, name)
            if t.numel() != x.shape[1]:
                raise RuntimeError(f"instance_norm: {name} has {t.numel()} elements, expected {x.shape[1]}")
    return _SpInstanceNormFn.apply(x, seg, int(nseg), weight, bias, eps)


# ---- a table against one row per scene: global pooling, broadcast, the squeeze-excite gate (csrc/sparse_global.hip) ----
BCAST_MODES = {"add": L.VDETR_BCAST_ADD, "mul": L.VDETR_BCAST_MUL, "cat": L.VDETR_BCAST_CAT}


def global_chunk_rows(N):
    """rows per chunk of the reducing launches of sparse_global.hip on a table of N rows"""
    return int(L.lib().vdetr_sp_global_chunk_rows(int(N)))


def _require_scene_table(op, x, seg, nseg, name="x"):
    L.require_gpu(x, name)
    L.require_float(x, name)
    L.require_contiguous(x, name)
    L.require_gpu(seg, "seg")
    L.require_int(seg, "seg")
    L.require_contiguous(seg, "seg")
    if x.dim() != 2 or seg.numel() != nseg + 1:
        raise RuntimeError(f"{op}: {name} must be [N, C] (it is {tuple(x.shape)}) and seg hold nseg + 1 = {nseg + 1} offsets "
                           f"(it holds {seg.numel()})")


def _require_scene_rows(op, g, nseg, name, C=None):
    L.require_gpu(g, name)
    L.require_float(g, name)
    L.require_contiguous(g, name)
    if g.dim() != 2 or g.shape[0] != nseg or (C is not None and g.shape[1] != C):
        raise RuntimeError(f"{op}: {name} is {tuple(g.shape)}, expected {(nseg, 'C' if C is None else C)}")


def _global_pool_desc(N, C, nseg, mode, seg, arg):
    d = L.SpGlobalPoolDesc()
    d.N, d.C, d.nseg, d.mode = N, C, nseg, mode
    d.seg, d.arg = seg.data_ptr(), L.ptr(arg).value
    return d


class _GlobalPoolFn(Function):
    """y [nseg, C] = sum / average / maximum of the rows seg[s] .. seg[s+1] of x (csrc/sparse_global.hip)."""

    @staticmethod
    def forward(ctx, x, seg, nseg, mode):
        N, C = x.shape
        lib = L.lib()
        new = torch.empty if N and nseg else torch.zeros  # (a table without rows launches nothing)
        y = new((nseg, C), dtype=torch.float32, device=x.device)
        arg = None
        if mode == L.VDETR_POOL_MAX:
            arg = torch.empty((nseg, C), dtype=torch.int32, device=x.device) if N and nseg else \
                torch.full((nseg, C), -1, dtype=torch.int32, device=x.device)
        ws = L.workspace(lib.vdetr_sp_global_pool_workspace_bytes(N, C, nseg), x.device)
        d = _global_pool_desc(N, C, nseg, mode, seg, arg)
        d.x, d.y, d.workspace = x.data_ptr(), y.data_ptr(), ws.data_ptr()
        L.check(lib.vdetr_sp_global_pool_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_global_pool_fwd")
        ctx.save_for_backward(seg, arg)
        ctx.cfg = (N, C, nseg, mode)
        if arg is not None:
            ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, dy, _darg):
        seg, arg = ctx.saved_tensors
        N, C, nseg, mode = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        dy = dy.contiguous()
        dx = (torch.empty if N and nseg else torch.zeros)((N, C), dtype=torch.float32, device=dy.device)
        d = _global_pool_desc(N, C, nseg, mode, seg, arg)
        L.check(L.lib().vdetr_sp_global_pool_bwd_f32(ctypes.byref(d), L.ptr(dy), L.ptr(dx), L.stream_ptr()), "sp_global_pool_bwd")
        return dx, None, None, None


def global_pool(x, seg, nseg, mode, return_arg=False):
    """Global pooling of a sparse tensor's table x [N, C] (contiguous fp32 on the device, C % 4 == 0, C <= 1024) over the scenes
    ``seg`` [nseg + 1] int32 (``scene_segments``; device, seg[0] = 0, seg[nseg] = N): mode "sum" | "avg" | "max" -> y [nseg, C].
    avg is the float32 sum times 1 / n; a scene without rows gives 0 in every mode and passes no gradient; max follows np.max /
    np.argmax (ties: the lowest row; a NaN wins).  ``return_arg``: also arg [nseg, C] int32, the absolute row of every maximum
    (-1: no row; None unless mode is "max").  Two launches forward, one backward; deterministic; no host read."""
    if mode not in POOL_MODES:
        raise ValueError(f"global_pool: mode {mode!r} (sum, avg, max)")
    _require_scene_table("global_pool", x, seg, nseg)
    y, arg = _GlobalPoolFn.apply(x, seg, int(nseg), POOL_MODES[mode])
    return (y, arg) if return_arg else y


def _broadcast_desc(N, Cx, Cg, nseg, mode, seg):
    d = L.SpBroadcastDesc()
    d.N, d.Cx, d.Cg, d.nseg, d.mode, d.relu = N, Cx, Cg, nseg, mode, 0
    d.seg = seg.data_ptr()
    return d


def _broadcast_forward(x, g, seg, nseg, mode, residual=None, relu=False):
    (N, Cx), Cg = x.shape, g.shape[1]
    y = torch.empty((N, Cx + Cg if mode == L.VDETR_BCAST_CAT else Cx), dtype=torch.float32, device=x.device)
    d = _broadcast_desc(N, Cx, Cg, nseg, mode, seg)
    d.relu = int(bool(relu))
    d.x, d.g, d.residual, d.y = x.data_ptr(), g.data_ptr(), L.ptr(residual).value, y.data_ptr()
    L.check(L.lib().vdetr_sp_broadcast_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_broadcast_fwd")
    return y


class _BroadcastFn(Function):
    """y = x + g[s] / x * g[s] / (x | g[s]) over the rows seg[s] .. seg[s+1] (csrc/sparse_global.hip)."""

    @staticmethod
    def forward(ctx, x, g, seg, nseg, mode):
        ctx.save_for_backward(x if mode == L.VDETR_BCAST_MUL else None, g if mode == L.VDETR_BCAST_MUL else None, seg)
        ctx.cfg = (x.shape[0], x.shape[1], g.shape[1], nseg, mode)
        return _broadcast_forward(x, g, seg, nseg, mode)

    @staticmethod
    def backward(ctx, dy):
        x, g, seg = ctx.saved_tensors
        N, Cx, Cg, nseg, mode = ctx.cfg
        need_x, need_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_g):
            return None, None, None, None, None
        dy = dy.contiguous()
        lib = L.lib()
        live = bool(N and nseg)
        dx = dg = ws = None
        if need_x:
            if mode == L.VDETR_BCAST_ADD:
                dx = dy  # (no launch: the gradient passes through)
            else:
                dx = (torch.empty if live else torch.zeros)((N, Cx), dtype=torch.float32, device=dy.device)
        if need_g:
            dg = (torch.empty if live else torch.zeros)((nseg, Cg), dtype=torch.float32, device=dy.device)
            ws = L.workspace(lib.vdetr_sp_broadcast_workspace_bytes(N, Cg, nseg), dy.device)
        launch_dx = dx if mode != L.VDETR_BCAST_ADD else None
        if launch_dx is not None or dg is not None:
            d = _broadcast_desc(N, Cx, Cg, nseg, mode, seg)
            d.x, d.g, d.workspace = L.ptr(x).value, L.ptr(g).value, L.ptr(ws).value
            L.check(lib.vdetr_sp_broadcast_bwd_f32(ctypes.byref(d), L.ptr(dy), L.ptr(launch_dx), L.ptr(dg), L.stream_ptr()),
                    "sp_broadcast_bwd")
        return dx, dg, None, None, None


def broadcast(x, g, seg, nseg, mode):
    """Broadcast of one row per scene over a sparse tensor's table: x [N, Cx], g [nseg, Cg] (contiguous fp32 on the device,
    widths multiples of 4 and <= 1024), ``seg`` [nseg + 1] int32 as in ``global_pool``; mode "add" | "mul" (Cg == Cx) -> [N, Cx],
    "cat" -> [N, Cx + Cg] = (x | g[s]).  One launch forward; backward: one sweep for dx that also leaves the partials of dg, and a
    fold (nothing is launched for a half nobody needs; the dx of "add" is dy itself).  Deterministic; no host read."""
    if mode not in BCAST_MODES:
        raise ValueError(f"broadcast: mode {mode!r} (add, mul, cat)")
    _require_scene_table("broadcast", x, seg, nseg)
    _require_scene_rows("broadcast", g, nseg, "g", None if mode == "cat" else x.shape[1])
    return _BroadcastFn.apply(x, g, seg, int(nseg), BCAST_MODES[mode])


def se_scale(x, seg, nseg, w1, b1, w2, b2, residual=None, relu=False):
    """The squeeze-excite layer of inference in three launches: x [N, C] * sigmoid(W2 relu(W1 avg_s(x) + b1) + b2)[s]
    (+ residual [N, C]) (then ReLU).  w1 [H, C], w2 [C, H] as nn.Linear holds them, H <= 256; b1 [H] / b2 [C] or None.  Launches:
    the pooling partials, the fold that goes on to the gate in the scene's workgroup, the broadcast multiply with its epilogue.
    No autograd: gradients do not flow through it."""
    _require_scene_table("se_scale", x, seg, nseg)
    N, C = x.shape
    if w1.dim() != 2 or w2.dim() != 2 or w1.shape[1] != C or tuple(w2.shape) != (C, w1.shape[0]):
        raise RuntimeError(f"se_scale: w1 is {tuple(w1.shape)} and w2 {tuple(w2.shape)}, expected [H, {C}] and [{C}, H]")
    H = w1.shape[0]
    for name, t, n in (("w1", w1, H * C), ("b1", b1, H), ("w2", w2, C * H), ("b2", b2, C), ("residual", residual, N * C)):
        if t is not None:
            L.require_gpu(t, name)
            L.require_float(t, name)
            L.require_contiguous(t, name)
            if t.numel() != n:
                raise RuntimeError(f"se_scale: {name} has {t.numel()} elements, expected {n}")
    lib = L.lib()
    nseg = int(nseg)
    gate = torch.empty((nseg, C), dtype=torch.float32, device=x.device)
    ws = L.workspace(lib.vdetr_sp_global_pool_workspace_bytes(N, C, nseg), x.device)
    d = L.SpSeGateDesc()
    d.N, d.C, d.H, d.nseg = N, C, H, nseg
    d.x, d.seg, d.gate, d.workspace = x.data_ptr(), seg.data_ptr(), gate.data_ptr(), ws.data_ptr()
    d.w1, d.b1, d.w2, d.b2 = w1.data_ptr(), L.ptr(b1).value, w2.data_ptr(), L.ptr(b2).value
    L.check(lib.vdetr_sp_se_gate_f32(ctypes.byref(d), L.stream_ptr()), "sp_se_gate")
    return _broadcast_forward(x, gate, seg, nseg, L.VDETR_BCAST_MUL, residual, relu)


# ---- sparse tensors on different key sets: union add / subtract and pruning (csrc/sparse_union.hip) ------------------
def union_tile():
    """keys per workgroup of the two map builders (the tests place their edge cases on its multiples)"""
    return int(L.lib().vdetr_sp_union_tile())


def _require_keys(t, name):
    L.require_gpu(t, name)
    L.require_contiguous(t, name)
    if t.dtype != torch.int64 or t.dim() != 1:
        raise RuntimeError(f"{name} must be a one-dimensional int64 key tensor (it is {t.dtype}, {tuple(t.shape)})")


def union_map(a_keys, b_keys):
    """The union of two sorted unique key sets (``pack_keys``) with its row maps: (u [nu] int64 ascending, row_a [na], row_b [nb]
    int32 = the position of every key in u, src_a [nu], src_b [nu] int32 = the row of a / b behind a row of u, or -1).  Equal to
    np.union1d / np.searchsorted bit for bit.  Two launches and ONE 4-byte read of nu behind them (geometry: the coordinate manager
    caches the map); u, src_a and src_b are views of buffers of na + nb entries."""
    _require_keys(a_keys, "a_keys")
    _require_keys(b_keys, "b_keys")
    if a_keys.device != b_keys.device:
        raise RuntimeError(f"union_map: a_keys on {a_keys.device}, b_keys on {b_keys.device}")
    na, nb, dev = a_keys.shape[0], b_keys.shape[0], a_keys.device
    if na + nb >= 2 ** 31:
        raise RuntimeError(f"union_map: {na} + {nb} keys are more than 31 bits hold")
    u = torch.empty(na + nb, dtype=torch.int64, device=dev)
    row_a, row_b = (torch.empty(n, dtype=torch.int32, device=dev) for n in (na, nb))
    src_a, src_b = (torch.empty(na + nb, dtype=torch.int32, device=dev) for _ in range(2))
    if na + nb == 0:
        return u, row_a, row_b, src_a, src_b
    lib = L.lib()
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.vdetr_sp_union_map_workspace_bytes(na, nb), dev)
    d = L.SpUnionMapDesc()
    d.na, d.nb = na, nb
    d.a, d.b, d.u = L.ptr(a_keys).value, L.ptr(b_keys).value, u.data_ptr()
    d.row_a, d.row_b, d.src_a, d.src_b = L.ptr(row_a).value, L.ptr(row_b).value, src_a.data_ptr(), src_b.data_ptr()
    d.count, d.workspace = count.data_ptr(), ws.data_ptr()
    L.check(lib.vdetr_sp_union_map_i64(ctypes.byref(d), L.stream_ptr()), "sp_union_map")
    nu = int(count)  # the size of the union is data: the one host read
    return u[:nu], row_a, row_b, src_a[:nu], src_b[:nu]


def prune_map(mask, keys):
    """The order-preserving compaction of the rows with ``mask`` true: (kept [nk] int32 ascending = np.nonzero(mask), pos [N] int32
    = the position of a row in kept or -1, keys_out [nk] = keys[kept]).  mask [N] bool and keys [N] int64 on the device.  Two
    launches and one 4-byte read of nk per call: the output shape is data."""
    _require_keys(keys, "keys")
    L.require_gpu(mask, "mask")
    L.require_contiguous(mask, "mask")
    if mask.dtype != torch.bool:
        raise RuntimeError(f"mask must be a bool tensor (it is {mask.dtype})")
    if mask.dim() != 1 or mask.shape[0] != keys.shape[0]:
        raise RuntimeError(f"prune_map: mask is {tuple(mask.shape)}, expected ({keys.shape[0]},): one entry per row")
    if mask.device != keys.device:
        raise RuntimeError(f"prune_map: mask on {mask.device}, keys on {keys.device}")
    N, dev = keys.shape[0], keys.device
    kept, pos = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    keys_out = torch.empty(N, dtype=torch.int64, device=dev)
    if N == 0:
        return kept, pos, keys_out
    lib = L.lib()
    count = torch.empty(1, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.vdetr_sp_prune_map_workspace_bytes(N), dev)
    d = L.SpPruneMapDesc()
    d.N, d.mask, d.keys = N, mask.data_ptr(), keys.data_ptr()
    d.kept, d.pos, d.keys_out, d.count, d.workspace = kept.data_ptr(), pos.data_ptr(), keys_out.data_ptr(), count.data_ptr(), ws.data_ptr()
    L.check(lib.vdetr_sp_prune_map_i64(ctypes.byref(d), L.stream_ptr()), "sp_prune_map")
    nk = int(count)
    return kept[:nk], pos, keys_out[:nk]


def _require_table(t, name):
    L.require_gpu(t, name)
    L.require_float(t, name)
    L.require_contiguous(t, name)
    if t.dim() != 2:
        raise RuntimeError(f"{name} must be a feature table [N, C] (it is {tuple(t.shape)})")


def _require_index(t, name, n=None):
    L.require_gpu(t, name)
    L.require_int(t, name)
    L.require_contiguous(t, name)
    if t.dim() != 1 or (n is not None and t.shape[0] != n):
        raise RuntimeError(f"{name} is {tuple(t.shape)}, expected ({'n' if n is None else n},)")


def _take_rows(x, idx, sign):
    nsrc, C = x.shape
    y = torch.empty((idx.shape[0], C), dtype=torch.float32, device=x.device)
    d = L.SpTakeRowsDesc()
    d.nrows, d.nsrc, d.C, d.sign = idx.shape[0], nsrc, C, sign
    d.x, d.idx, d.y = L.ptr(x).value, L.ptr(idx).value, L.ptr(y).value
    L.check(L.lib().vdetr_sp_take_rows_f32(ctypes.byref(d), L.stream_ptr()), "sp_take_rows")
    return y


class _TakeRowsFn(Function):
    """y[r] = sign * x[idx[r]] (0 where idx[r] < 0); backward: the same launch through ``back``, the inverse of ``idx``."""

    @staticmethod
    def forward(ctx, x, idx, back, sign):
        ctx.save_for_backward(back)
        ctx.sign = sign
        return _take_rows(x, idx, sign)

    @staticmethod
    def backward(ctx, dy):
        (back,) = ctx.saved_tensors
        return _take_rows(dy.contiguous(), back, ctx.sign), None, None, None


def take_rows(x, idx, back=None, sign=1):
    """y [R, C] = sign * x[idx[r]], an exact zero where idx[r] < 0.  x [N, C] contiguous fp32 on the device (C % 4 == 0), idx [R]
    int32 holding every row of x AT MOST ONCE, sign 1 or -1.  One launch.  Gradients reach x only with ``back`` [N] int32, the
    inverse of idx (back[i] = the r with idx[r] == i, or -1): the backward is this launch through it (the pruning's kept / pos, the
    union's src / row)."""
    _require_table(x, "x")
    _require_index(idx, "idx")
    if sign not in (1, -1):
        raise ValueError(f"take_rows: sign {sign!r} (1 or -1)")
    if back is None:
        if x.requires_grad and torch.is_grad_enabled():
            raise RuntimeError("take_rows: gradients of x need `back`, the inverse of idx")
        return _take_rows(x, idx, sign)
    _require_index(back, "back", x.shape[0])
    return _TakeRowsFn.apply(x, idx, back, sign)


class _UnionAddFn(Function):
    """y [nu, C] = a-or-zero + sign * b-or-zero on the union of two key sets; dA = dY[row_a], dB = sign * dY[row_b] (gathers)."""

    @staticmethod
    def forward(ctx, fa, fb, row_a, row_b, src_a, src_b, sign):
        nu, C = src_a.shape[0], fa.shape[1]
        y = torch.empty((nu, C), dtype=torch.float32, device=fa.device)
        d = L.SpUnionAddDesc()
        d.nu, d.na, d.nb, d.C, d.sign = nu, fa.shape[0], fb.shape[0], C, sign
        d.a, d.b, d.src_a, d.src_b, d.y = L.ptr(fa).value, L.ptr(fb).value, L.ptr(src_a).value, L.ptr(src_b).value, L.ptr(y).value
        L.check(L.lib().vdetr_sp_union_add_f32(ctypes.byref(d), L.stream_ptr()), "sp_union_add")
        ctx.save_for_backward(row_a, row_b)
        ctx.sign = sign
        return y

    @staticmethod
    def backward(ctx, dy):
        row_a, row_b = ctx.saved_tensors
        dy = dy.contiguous()
        da = _take_rows(dy, row_a, 1) if ctx.needs_input_grad[0] else None
        db = _take_rows(dy, row_b, ctx.sign) if ctx.needs_input_grad[1] else None
        return da, db, None, None, None, None, None


def union_add(fa, fb, row_a, row_b, src_a, src_b, sign=1):
    """y [nu, C] on the union of two key sets (``union_map``): row u is fa's row, zero where a has no such site, plus (sign 1) or
    minus (sign -1) fb's row, likewise — one fp32 add or subtract of two selected operands.  fa [na, C], fb [nb, C] contiguous fp32
    on the device, C % 4 == 0.  One launch forward, at most two backward (gathers through row_a / row_b); deterministic."""
    _require_table(fa, "fa")
    _require_table(fb, "fb")
    if fa.shape[1] != fb.shape[1]:
        raise ValueError(f"union_add: {fa.shape[1]} and {fb.shape[1]} channels")
    if sign not in (1, -1):
        raise ValueError(f"union_add: sign {sign!r} (1 or -1)")
    _require_index(row_a, "row_a", fa.shape[0])
    _require_index(row_b, "row_b", fb.shape[0])
    _require_index(src_a, "src_a")
    _require_index(src_b, "src_b", src_a.shape[0])
    return _UnionAddFn.apply(fa, fb, row_a, row_b, src_a, src_b, sign)


# ---- voxelisation: keys, sites and the quantisation modes (csrc/sparse_voxel.hip) ------------------------------------
VOXEL_MODES = {"sum": L.VDETR_VOXEL_SUM, "average": L.VDETR_VOXEL_AVG, "max": L.VDETR_VOXEL_MAX, "first": L.VDETR_VOXEL_FIRST}
RANGE_MESSAGE = "voxel coordinates outside the 16-bit key range"


def voxel_tile():
    """sorted keys per workgroup of the sites pass (the tests place their edge cases on its multiples)"""
    return int(L.lib().vdetr_sp_voxel_tile())


class VoxelMap(tuple):
    """(sites [M] int64 ascending unique keys, inverse [N] int32 = the site row of every input row, first [M] int64 = the lowest
    input row of each site, seg [M + 1] int32 = the run starts in sorted order, order [N] int32 = the stable sort's permutation).
    ``num_scenes`` is the B of the offsets; for ready coordinates the highest batch index + 1, which rides with the one host read."""
    num_scenes = None

    sites, inverse, first, seg, order = (property(lambda self, i=i: self[i]) for i in range(5))


def _voxel_sites(keys, num_scenes):
    """the shared second half of ``voxel_map`` / ``voxel_map_coords``: stable sort, the two sites launches, the ONE host read"""
    N, dev = keys.shape[0], keys.device
    sites = torch.empty(N, dtype=torch.int64, device=dev)
    first = torch.empty(N, dtype=torch.int64, device=dev)
    inverse, order32 = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    seg = torch.empty(N + 1, dtype=torch.int32, device=dev)
    if N == 0:
        seg.zero_()
        vm = VoxelMap((sites, inverse, first, seg, order32))
        vm.num_scenes = num_scenes or 0
        return vm
    sorted_keys, order = torch.sort(keys, stable=True)
    lib = L.lib()
    count = torch.empty(2, dtype=torch.int32, device=dev)
    ws = L.workspace(lib.vdetr_sp_voxel_sites_workspace_bytes(N), dev)
    d = L.SpVoxelSitesDesc()
    d.N, d.sorted, d.order = N, sorted_keys.data_ptr(), order.data_ptr()
    d.sites, d.first, d.inverse, d.order32, d.seg = (t.data_ptr() for t in (sites, first, inverse, order32, seg))
    d.count, d.workspace = count.data_ptr(), ws.data_ptr()
    L.check(lib.vdetr_sp_voxel_sites_i64(ctypes.byref(d), L.stream_ptr()), "sp_voxel_sites")
    # the number of sites is data: the one host read (eight bytes).  The range flag rides with it as -1; otherwise the word
    # is the highest batch index + 1, the scene count of a map built from ready coordinates
    M, scenes = count.tolist()
    if scenes < 0:
        raise ValueError(f"{RANGE_MESSAGE} (a voxel index outside [{-KEY_BIAS}, {KEY_BIAS - 1}], a non-finite coordinate or a "
                         f"batch index outside [0, 32767])")
    vm = VoxelMap((sites[:M], inverse, first[:M], seg[:M + 1], order32))
    vm.num_scenes = scenes if num_scenes is None else num_scenes
    return vm


def voxel_map(points, offsets, voxel_size):
    """Packed points [N, >= 3] fp32 on the device (unit column stride; only the first three columns are read), offsets [B + 1]
    (host sequence, or an int32 device tensor) and the voxel size (a Python float) -> ``VoxelMap``.  The voxel index of a point is,
    bit for bit, ``torch.floor(points[:, :3] / voxel_size).to(torch.int32)`` on the device.  One keys launch, a stable library
    sort, two sites launches and ONE host read of eight bytes (the site count and the range flag); a raised flag is the
    ValueError of ``pack_keys``."""
    L.require_float(points, "points")
    if points.dim() != 2 or points.shape[1] < 3 or (points.shape[0] > 1 and points.stride(0) < 3) or \
            (points.shape[0] > 0 and points.stride(1) != 1):
        raise RuntimeError(f"points must be [N, 3 or more columns] with unit column stride (it is {tuple(points.shape)})")
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and voxel_size < float("inf")):
        raise ValueError(f"voxel_map: voxel_size {voxel_size!r} must be positive and finite")
    L.require_gpu(points, "points")
    N, dev = points.shape[0], points.device
    if N >= 2 ** 31:
        raise RuntimeError(f"voxel_map: {N} points are more than 31 bits hold")
    if torch.is_tensor(offsets):
        L.require_int(offsets, "offsets")
        L.require_contiguous(offsets, "offsets")
        if offsets.dim() != 1 or offsets.shape[0] < 2:
            raise ValueError("offsets must hold B + 1 row offsets")
        off_dev = offsets if offsets.is_cuda else offsets.to(dev, non_blocking=True)
    else:
        off = np.ascontiguousarray(np.asarray(offsets), dtype=np.int64)
        if off.ndim != 1 or len(off) < 2:
            raise ValueError("offsets must hold B + 1 row offsets")
        if off[0] != 0 or off[-1] != N or (np.diff(off) < 0).any():
            raise ValueError(f"offsets run from {off[0]} to {off[-1]}, points has {N} rows")
        off_dev = torch.from_numpy(off.astype(np.int32)).to(dev, non_blocking=True)
    B = off_dev.shape[0] - 1
    if B > 32768:
        raise ValueError(f"{RANGE_MESSAGE}: {B} scenes")
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    if N:
        d = L.SpVoxelKeysDesc()
        d.N, d.B, d.stride, d.voxel_size = N, B, points.stride(0) if N > 1 else points.shape[1], voxel_size
        d.points, d.offsets, d.coords, d.keys = points.data_ptr(), off_dev.data_ptr(), None, keys.data_ptr()
        L.check(L.lib().vdetr_sp_voxel_keys_f32(ctypes.byref(d), L.stream_ptr()), "sp_voxel_keys")
    return _voxel_sites(keys, B)


def voxel_map_coords(coords):
    """Ready integer coordinates [N, 4] (batch, x, y, z) on the device -> ``VoxelMap`` (see ``voxel_map``)."""
    if coords.dim() != 2 or coords.shape[1] != 4:
        raise RuntimeError(f"coords must be [N, 4] (batch, x, y, z) (it is {tuple(coords.shape)})")
    if coords.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise RuntimeError(f"coords must be an integer tensor (it is {coords.dtype})")
    L.require_gpu(coords, "coords")
    if coords.dtype != torch.int32:
        # (what no key holds stays outside after the clamp)
        coords = coords.clamp(-(1 << 20), 1 << 20).to(torch.int32) if coords.dtype == torch.int64 else coords.to(torch.int32)
    coords = coords.contiguous()
    N, dev = coords.shape[0], coords.device
    if N >= 2 ** 31:
        raise RuntimeError(f"voxel_map_coords: {N} points are more than 31 bits hold")
    keys = torch.empty(N, dtype=torch.int64, device=dev)
    if N:
        d = L.SpVoxelKeysDesc()
        d.N, d.points, d.offsets, d.coords, d.keys = N, None, None, coords.data_ptr(), keys.data_ptr()
        L.check(L.lib().vdetr_sp_voxel_keys_f32(ctypes.byref(d), L.stream_ptr()), "sp_voxel_keys")
    return _voxel_sites(keys, None)


def region_keys(keys, offsets):
    """The sites a kernel region reaches from a key set: sorted unique ``keys`` [N] int64 and ``offsets`` [K, 3]
    int32, both on the device, the offsets already scaled and signed -> the sorted unique int64 keys of every ``site + offset``.
    One candidates launch (csrc/sparse_voxel.hip: no atomics, no memset), the stable library sort, the two sites launches of
    ``voxel_map`` and their ONE host read of eight bytes (the site count and the range flag).  A candidate outside the 16-bit
    fields raises the ValueError of ``voxel_map``."""
    L.require_gpu(keys, "keys")
    L.require_gpu(offsets, "offsets")
    if keys.dtype != torch.int64 or keys.dim() != 1:
        raise RuntimeError(f"keys must be a 1-D int64 tensor (it is {tuple(keys.shape)} {keys.dtype})")
    if offsets.dtype != torch.int32 or offsets.dim() != 2 or offsets.shape[1] != 3:
        raise RuntimeError(f"offsets must be a [K, 3] int32 tensor (it is {tuple(offsets.shape)} {offsets.dtype})")
    keys, offsets = keys.contiguous(), offsets.contiguous()
    N, K = keys.shape[0], offsets.shape[0]
    if K * N >= 2 ** 31:
        raise RuntimeError(f"region_keys: {K} offsets x {N} sites are more candidates than 31 bits hold")
    cand = torch.empty(K * N, dtype=torch.int64, device=keys.device)
    if K * N:
        d = L.SpRegionKeysDesc()
        d.N, d.K, d.keys, d.offsets, d.cand = N, K, keys.data_ptr(), offsets.data_ptr(), cand.data_ptr()
        L.check(L.lib().vdetr_sp_region_keys_i64(ctypes.byref(d), L.stream_ptr()), "sp_region_keys")
    return _voxel_sites(cand, None).sites.clone()  # (the sites pass writes into a buffer of K * N: keep the M that are sites)


def target_keys(coordinates):
    """Caller-chosen output sites: integer coordinates [M, 4] (batch, x, y, z) on the device -> (keys sorted and unique, inverse
    [M] int32 = the key row of every given coordinate).  ``voxel_map_coords`` under the name of its use here: one keys launch,
    the sort, the sites pass, one host read."""
    vm = voxel_map_coords(coordinates)
    return vm.sites, vm.inverse


def _require_vmap(vmap, n=None):
    if not isinstance(vmap, tuple) or len(vmap) != 5:
        raise RuntimeError("vmap must be the (sites, inverse, first, seg, order) of voxel_map / voxel_map_coords")
    sites, inverse, first, seg, order = vmap
    _require_keys(sites, "sites")
    _require_index(inverse, "inverse", n)
    _require_index(order, "order", inverse.shape[0])
    _require_index(seg, "seg", sites.shape[0] + 1)
    return sites.shape[0], inverse.shape[0]


def _voxel_reduce_launch(x, order, seg, M, mode):
    N, C = x.shape
    y = torch.empty((M, C), dtype=torch.float32, device=x.device)
    arg = torch.empty((M, C), dtype=torch.int32, device=x.device) if mode == L.VDETR_VOXEL_MAX else None
    d = L.SpVoxelReduceDesc()
    d.M, d.N, d.C, d.mode = M, N, C, mode
    d.x, d.order, d.seg, d.y, d.arg = L.ptr(x).value, L.ptr(order).value, L.ptr(seg).value, L.ptr(y).value, L.ptr(arg).value
    L.check(L.lib().vdetr_sp_voxel_reduce_f32(ctypes.byref(d), L.stream_ptr()), "sp_voxel_reduce")
    return y, arg


class _VoxelReduceFn(Function):
    """y [M, C] = the fold of x [N, C] over the points of every site (csrc/sparse_voxel.hip); dx is a gather through ``inverse``."""

    @staticmethod
    def forward(ctx, x, inverse, seg, order, M, mode):
        y, arg = _voxel_reduce_launch(x, order, seg, M, mode)
        ctx.save_for_backward(inverse, seg, order, arg)
        ctx.cfg = (M, x.shape[0], x.shape[1], mode)
        if arg is None:
            return y, None
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, dy, _darg):
        inverse, seg, order, arg = ctx.saved_tensors
        M, N, C, mode = ctx.cfg
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        dy = dy.contiguous()
        dx = torch.empty((N, C), dtype=torch.float32, device=dy.device)
        d = L.SpVoxelReduceDesc()
        d.M, d.N, d.C, d.mode = M, N, C, mode
        d.order, d.seg, d.arg = L.ptr(order).value, L.ptr(seg).value, L.ptr(arg).value
        L.check(L.lib().vdetr_sp_voxel_reduce_grad_f32(ctypes.byref(d), L.ptr(dy), L.ptr(inverse), L.ptr(dx), L.stream_ptr()),
                "sp_voxel_reduce_grad")
        return dx, None, None, None, None, None


def voxel_reduce(features, vmap, mode, return_arg=False):
    """The features of the sites of a ``VoxelMap``: features [N, C] contiguous fp32 on the device (any C >= 1), mode "sum" |
    "average" | "max" | "first" -> [M, C].  A site's value is the float32 fold of its points in ascending input-row order
    (average: one division by the count behind the sum; max: np.maximum, a NaN wins, ties keep the lower row; first: the lowest
    row, MinkowskiEngine's RANDOM_SUBSAMPLE): two runs agree bit for bit.  One launch forward, one backward (a gather); no atomics.
    ``return_arg``: also the winning input row per (site, channel) [M, C] int32 (max; None otherwise)."""
    _require_table(features, "features")
    if mode not in VOXEL_MODES:
        raise ValueError(f"voxel_reduce: mode {mode!r} (sum, average, max, first)")
    M, N = _require_vmap(vmap, features.shape[0])
    if features.shape[1] < 1:
        raise RuntimeError(f"features must be a feature table [N, C] with C >= 1 (it is {tuple(features.shape)})")
    _, inverse, _, seg, order = vmap
    y, arg = _VoxelReduceFn.apply(features, inverse, seg, order, M, VOXEL_MODES[mode])
    return (y, arg) if return_arg else y


class _VoxelSliceFn(Function):
    """y [N, C] = x[inverse] (site features back on the points); backward: the sum fold of dy over every site's points."""

    @staticmethod
    def forward(ctx, x, inverse, seg, order):
        ctx.save_for_backward(inverse, seg, order)
        ctx.M = x.shape[0]
        N, C = inverse.shape[0], x.shape[1]
        dx = torch.empty((N, C), dtype=torch.float32, device=x.device)
        d = L.SpVoxelReduceDesc()  # the sum mode's gradient launch IS the row gather through `inverse`, at any width
        d.M, d.N, d.C, d.mode = ctx.M, N, C, L.VDETR_VOXEL_SUM
        d.seg = L.ptr(seg).value
        L.check(L.lib().vdetr_sp_voxel_reduce_grad_f32(ctypes.byref(d), L.ptr(x), L.ptr(inverse), L.ptr(dx), L.stream_ptr()),
                "sp_voxel_reduce_grad")
        return dx

    @staticmethod
    def backward(ctx, dy):
        inverse, seg, order = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        return _voxel_reduce_launch(dy.contiguous(), order, seg, ctx.M, L.VDETR_VOXEL_SUM)[0], None, None, None


def voxel_slice(site_features, vmap):
    """[N, C] = site_features[inverse]: the features of every point's site (site_features [M, C] contiguous fp32 on the device).
    One gather launch; the backward is the sum fold in the fixed order of ``voxel_reduce``."""
    _require_table(site_features, "site_features")
    M, _ = _require_vmap(vmap)
    if site_features.shape[0] != M:
        raise RuntimeError(f"voxel_slice: site_features has {site_features.shape[0]} rows, the map {M} sites")
    _, inverse, _, seg, order = vmap
    return _VoxelSliceFn.apply(site_features, inverse, seg, order)


def voxel_labels(labels, vmap, ignore_label=-100):
    """[M] the label all points of a site share, ``ignore_label`` where they differ (labels [N] integer, on the device; the
    result has the labels' dtype).  One launch."""
    if labels.dtype not in (torch.int32, torch.int64) or labels.dim() != 1:
        raise RuntimeError(f"labels must be a one-dimensional int32 or int64 tensor (it is {labels.dtype}, {tuple(labels.shape)})")
    L.require_gpu(labels, "labels")
    M, N = _require_vmap(vmap, labels.shape[0])
    _, _, _, seg, order = vmap
    lab = labels.to(torch.int32).contiguous()
    out = torch.empty(M, dtype=torch.int32, device=labels.device)
    L.check(L.lib().vdetr_sp_voxel_labels_i32(L.ptr(lab), L.ptr(order), L.ptr(seg), M, N, int(ignore_label), L.ptr(out), L.stream_ptr()),
            "sp_voxel_labels")
    return out.to(labels.dtype)


# ---- trilinear interpolation at float coordinates (csrc/sparse_interp.hip) -------------------------------------------
def interp_tile():
    """points per workgroup of the map launch (the tests place their edge cases on its multiples)"""
    return int(L.lib().vdetr_sp_interp_tile())


class InterpMap:
    """The geometry of one interpolation, reusable for any feature table on the same keys: ``nbr`` [N, 8] int32 = the site row of
    every corner (k = 4 bx + 2 by + bz, bit 1 = the upper site) or -1, ``w`` [N, 8] fp32 = its trilinear weight (0 where absent),
    ``M`` sites, ``N`` points.  ``order`` [8 N] / ``seg`` [M + 1] int32, the pairs grouped by site in ascending (n, k) for the
    backward, are built on first use: a stable library sort and one launch, no host read."""

    def __init__(self, nbr, w, M):
        self.nbr, self.w, self.M, self.N = nbr, w, int(M), nbr.shape[0]
        self._fold = None

    def _folded(self):
        if self._fold is None:
            dev = self.nbr.device
            order32 = torch.empty(8 * self.N, dtype=torch.int32, device=dev)
            seg = torch.empty(self.M + 1, dtype=torch.int32, device=dev)
            # absent pairs (-1) sort first; the stable sort keeps every site's pairs in ascending (n, k)
            rows, order = torch.sort(self.nbr.view(-1), stable=True) if self.N else (None, None)
            L.check(L.lib().vdetr_sp_interp_seg_i32(L.ptr(rows), L.ptr(order), self.M, self.N, L.ptr(order32), L.ptr(seg), L.stream_ptr()),
                    "sp_interp_seg")
            self._fold = (order32, seg)
        return self._fold

    order = property(lambda self: self._folded()[0])
    seg = property(lambda self: self._folded()[1])


def interp_map(keys, tensor_stride, tfield):
    """keys [M] sorted unique int64 (``pack_keys``) of a sparse tensor at integer ``tensor_stride`` s >= 1 and tfield [N, 4] fp32
    (batch, x, y, z) in units of the finest voxel, both on the device -> ``InterpMap``.  A site's feature sits at its integer
    coordinate; per axis lo = floor_div(floor(x), s) * s and t = (x - lo) / s, the corners are the sites (lo | lo + s) on every
    axis.  A point outside every key (non-finite, outside the 16-bit range, a batch value that is no integer in [0, 32767]) has
    eight absent corners; nothing is raised and nothing is read back.  One launch."""
    # (the checks that do not need the tensors on a device come first)
    if keys.dtype != torch.int64 or keys.dim() != 1:
        raise RuntimeError(f"keys must be a one-dimensional int64 key tensor (it is {keys.dtype}, {tuple(keys.shape)})")
    if not isinstance(tensor_stride, (int, np.integer)) or isinstance(tensor_stride, bool) or not 1 <= tensor_stride <= KEY_BIAS:
        raise ValueError(f"interp_map: tensor_stride {tensor_stride!r} must be an integer in [1, {KEY_BIAS}]")
    L.require_float(tfield, "tfield")
    if tfield.dim() != 2 or tfield.shape[1] != 4:
        raise RuntimeError(f"tfield must be [N, 4] (batch, x, y, z) (it is {tuple(tfield.shape)})")
    _require_keys(keys, "keys")
    L.require_gpu(tfield, "tfield")
    L.require_contiguous(tfield, "tfield")
    if tfield.device != keys.device:
        raise RuntimeError(f"interp_map: keys on {keys.device}, tfield on {tfield.device}")
    M, N, dev = keys.shape[0], tfield.shape[0], keys.device
    if 8 * N >= 2 ** 31:
        raise RuntimeError(f"interp_map: 8 x {N} pairs are more than 31 bits hold")
    nbr = torch.empty((N, 8), dtype=torch.int32, device=dev)
    w = torch.empty((N, 8), dtype=torch.float32, device=dev)
    d = L.SpInterpMapDesc()
    d.M, d.N, d.stride = M, N, int(tensor_stride)
    d.keys, d.tfield, d.nbr, d.w = L.ptr(keys).value, L.ptr(tfield).value, L.ptr(nbr).value, L.ptr(w).value
    L.check(L.lib().vdetr_sp_interp_map_f32(ctypes.byref(d), L.stream_ptr()), "sp_interp_map")
    return InterpMap(nbr, w, M)


class _InterpFn(Function):
    """y [N, C] = sum_k w[n, k] * x[nbr[n, k]]; dx [M, C] = the same pairs folded per site in ascending (n, k) (no atomics)."""

    @staticmethod
    def forward(ctx, x, imap):
        ctx.imap = imap
        M, C = x.shape
        y = torch.empty((imap.N, C), dtype=torch.float32, device=x.device)
        d = L.SpInterpDesc()
        d.M, d.N, d.C = M, imap.N, C
        d.x, d.nbr, d.w, d.y = L.ptr(x).value, L.ptr(imap.nbr).value, L.ptr(imap.w).value, L.ptr(y).value
        L.check(L.lib().vdetr_sp_interp_fwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_interp_fwd")
        return y

    @staticmethod
    def backward(ctx, dy):
        imap = ctx.imap
        if not ctx.needs_input_grad[0]:
            return None, None
        dy = dy.contiguous()
        C = dy.shape[1]
        dx = torch.empty((imap.M, C), dtype=torch.float32, device=dy.device)
        d = L.SpInterpDesc()
        d.M, d.N, d.C = imap.M, imap.N, C
        d.x, d.w, d.order, d.seg, d.y = L.ptr(dy).value, L.ptr(imap.w).value, L.ptr(imap.order).value, L.ptr(imap.seg).value, L.ptr(dx).value
        L.check(L.lib().vdetr_sp_interp_bwd_f32(ctypes.byref(d), L.stream_ptr()), "sp_interp_bwd")
        return dx, None


def interpolate(feats, imap):
    """[N, C] = the trilinear interpolation of feats [M, C] (contiguous fp32 on the device, any C >= 1) at the points of an
    ``InterpMap``: the weighted sum of the corners that exist, in ascending corner order, without renormalisation (a point with
    no site around it reads zeros).  One launch forward; the backward is one launch (plus, once per map, a stable sort and the
    segment launch) and folds every site's pairs in ascending (point, corner) order: no atomics, two runs agree bit for bit."""
    if not isinstance(imap, InterpMap):
        raise RuntimeError("imap must be the InterpMap of interp_map")
    L.require_float(feats, "feats")
    if feats.dim() != 2 or feats.shape[1] < 1:
        raise RuntimeError(f"feats must be a feature table [M, C] with C >= 1 (it is {tuple(feats.shape)})")
    if feats.shape[0] != imap.M:
        raise RuntimeError(f"interpolate: feats has {feats.shape[0]} rows, the map {imap.M} sites")
    _require_table(feats, "feats")
    if feats.device != imap.nbr.device:
        raise RuntimeError(f"interpolate: feats on {feats.device}, the map on {imap.nbr.device}")
    return _InterpFn.apply(feats, imap)


_MODE = os.environ.get("VDETR_SP_MODE", "pairs")  # pairs (fused kernels) | plan (batched library GEMMs) | im2col
_IM2COL = _MODE == "im2col" or os.environ.get("VDETR_SP_IM2COL", "0") == "1"  # A/B switch: one dense im2col GEMM per layer instead of the plan


def sparse_conv(feats, weight, nbr, inv, plan=None):
    """feats [Nin, Cin] (any Cin: padded to a multiple of 4 here), weight [K, Cin, Cout], nbr [K, Nout], inv [K, Nin];
    ``plan``: the ConvPlan of (nbr, Nin) if the caller caches it (the coordinate manager does)."""
    cin, cout = feats.shape[1], weight.shape[2]
    if isinstance(plan, PairPlan) or (plan is None and _MODE == "pairs"):
        if plan is None:
            plan = PairPlan(nbr, feats.shape[0])
        feats, weight = _pair_operands(feats, weight)
        out = _PairsConvFn.apply(feats, weight, plan)
        return out[:, :cout] if out.shape[1] != cout else out
    pad = (-cin) % 4
    if pad:
        feats = torch.nn.functional.pad(feats, (0, pad))
        weight = torch.nn.functional.pad(weight, (0, 0, 0, pad))
    if _IM2COL:
        return _SparseConvFn.apply(feats.contiguous(), weight, nbr, inv)
    if plan is None:
        plan = ConvPlan(nbr, feats.shape[0])
    return _PlannedConvFn.apply(feats.contiguous(), weight, plan)
