"""The library's dropout generator (csrc/drop_stream.h) restated in numpy, and one function per stream that returns the keep mask a
kernel must draw: tests/test_drop_stream.py pins this file to known answers on the CPU, tests/test_gpu_drop_stream.py holds the
masks the kernels return to it.  Nothing here touches the GPU or the code under test.

32-bit words travel as uint64 arrays masked to 32 bits (a product of two of them fits).  A stream `g` is the tuple (seed_lo,
seed_hi, off_lo, off_hi) that `stream` folds from the by-value {seed, offset} and the optional device state.
"""
import numpy as np

from norm_cases import drop_threshold

_M32 = np.uint64(0xFFFFFFFF)
_M64 = (1 << 64) - 1


def _u32(x):
    return np.asarray(x).astype(np.uint64) & _M32


def _mul(x, c):
    return (_u32(x) * np.uint64(c)) & _M32


def fmix32(x):
    """MurmurHash3's 32-bit finaliser"""
    x = _u32(x)
    x = x ^ (x >> np.uint64(16))
    x = _mul(x, 0x85EBCA6B)
    x = x ^ (x >> np.uint64(13))
    x = _mul(x, 0xC2B2AE35)
    return x ^ (x >> np.uint64(16))


def stream(seed, offset=0, state=None):
    """seed ^= state.seed, offset += state.offset (mod 2^64), split into 32-bit halves"""
    s, o = int(seed) & _M64, int(offset) & _M64
    if state is not None:
        s ^= int(state[0]) & _M64
        o = (o + (int(state[1]) & _M64)) & _M64
    return tuple(np.uint64(v) for v in (s & 0xFFFFFFFF, s >> 32, o & 0xFFFFFFFF, o >> 32))


def prefix(g, major, minor):
    x = fmix32(((_mul(major, 0x9E3779B1) + g[2]) & _M32) ^ g[0])
    return fmix32(x ^ ((_mul(minor, 0x27D4EB2F) + g[3]) & _M32) ^ g[1])


def word(pre, j):
    return fmix32(_u32(pre) ^ _mul(j, 0x165667B1))


def successor(x):
    return fmix32((_u32(x) + np.uint64(0x9E3779B9)) & _M32)


def flat(g, i):
    """the first word of float4 number i of a flat tensor (i a non-negative 64-bit index)"""
    i = np.asarray(i).astype(np.uint64)
    x = fmix32(((_mul(i & _M32, 0x9E3779B1) + g[2]) & _M32) ^ g[0] ^ _mul(i >> np.uint64(32), 0x27D4EB2F))
    return fmix32(x ^ g[1] ^ g[3])


def draws4(x):
    """[..., 4]: low and high half of x, then of its successor"""
    y = successor(x)
    return np.stack((x & np.uint64(0xFFFF), x >> np.uint64(16), y & np.uint64(0xFFFF), y >> np.uint64(16)), -1)


# ---- the four streams: boolean keep masks (draw >= threshold; everything without dropout) ---------------------------------------
def keep_add_ln(rows, C, p, g):
    """add_ln.hip, rowblock.hip: major row, minor 1, word channel / 4, four draws -> [rows, C]"""
    x = word(prefix(g, np.arange(rows), 1)[:, None], np.arange(C // 4)[None, :])
    return draws4(x).reshape(rows, C) >= drop_threshold(p)


def keep_bn(B, C, N, p, g):
    """bn_act.hip, heads.hip: major channel, minor 1, element e = b N + i of the channel, pair word e >> 1 -> [B, C, N]"""
    e = np.arange(B * N)
    x = word(prefix(g, np.arange(C), 1)[:, None], (e >> 1)[None, :])
    draw = np.where(e & 1, x >> np.uint64(16), x & np.uint64(0xFFFF))
    return (draw >= drop_threshold(p)).reshape(C, B, N).transpose(1, 0, 2)


def keep_flat(n, p, g):
    """relu_dropout (bn_act.hip, rowblock.hip): float4 number i of the flat tensor -> [n], n a multiple of 4"""
    return draws4(flat(g, np.arange(n // 4))).reshape(n) >= drop_threshold(p)


def keep_attention(B, H, nQ, nK, p, g):
    """attn_*.hip: major query, minor b * 64 + (h >> 2), word key, draw h & 3 -> [B, H, nQ, nK]"""
    b, h, q = np.arange(B)[:, None, None], np.arange(H)[None, :, None], np.arange(nQ)[None, None, :]
    pre = prefix(g, q + 0 * b + 0 * h, b * 64 + (h >> 2) + 0 * q)
    d = draws4(word(pre[..., None], np.arange(nK)))  # [B, H, nQ, nK, 4]
    pick = np.broadcast_to((np.arange(H) & 3)[None, :, None, None, None], d.shape[:-1] + (1,))
    return np.take_along_axis(d, pick, -1)[..., 0] >= drop_threshold(p)
