"""The `guarded` fixture: every workspace the package asks `_lib.workspace` for comes out of a poisoned, guarded allocation.

A request of n bytes gets an allocation of 256 + front + n + tail bytes filled with 0xA5.  The n-byte view that is handed out
starts `front` bytes past a multiple of 256 B of the allocation's own address, so it is off the 256-B grid whatever the
allocator's alignment is, and it is filled with 0xFF: a word the library reads before it wrote it is a NaN as a float and -1 as
an int, and shows in the results.  After the op every byte in front of the view and every byte behind it must still read 0xA5.

`front` is 8 for the layouts that round the start themselves (csrc/workspace.h: any pointer is allowed) and 16 for the layouts
whose descriptor carries a bare pointer (their contract is 16-B alignment; the point is the bounds, not misaligned vector
accesses).  `tail` is 256 B or one whole further unit of the op's layout (a partial, a chunk, a tile's record), whichever is
larger: a count that is off by one lands inside the guard instead of flying past it.

A plain module, not a conftest: a test file imports the fixture by name.  It works on CPU tensors too (the self-test)."""
import pytest
import torch

GUARD, POISON = 0xA5, 0xFF


class Guard:
    """_lib.workspace's stand-in.  guard.layout(front, unit) sets the offsets of the workspaces handed out from then on; guard()
    synchronises, checks the guard bytes of every workspace handed out so far and answers how many there were."""

    def __init__(self):
        self.made = []  # (raw, lo, n, front): the allocation, the view's first byte in it, the view's length, its offset off the grid
        self.front, self.tail = 8, 256

    def layout(self, front=8, unit=0):
        assert front in (8, 16), "8: any pointer is allowed; 16: the bare-pointer layouts' contract"
        self.front, self.tail = front, max(256, int(unit))
        return self

    def workspace(self, nbytes, device):
        n = max(int(nbytes), 1)
        raw = torch.full((256 + self.front + n + self.tail,), GUARD, dtype=torch.uint8, device=device)
        lo = (-raw.data_ptr()) % 256 + self.front
        view = raw[lo:lo + n]
        view.fill_(POISON)
        self.made.append((raw, lo, n, self.front))
        return view

    def block(self, i):
        """workspace i with its guards, as a view: `front` guard bytes, the n bytes handed out, the tail guard"""
        raw, lo, n, front = self.made[i]
        return raw[lo - front:]

    def interior(self, i):
        """the bytes of workspace i as the op left them (a copy)"""
        raw, lo, n, _ = self.made[i]
        return raw[lo:lo + n].clone()

    def __call__(self):
        if any(m[0].is_cuda for m in self.made):
            torch.cuda.synchronize()
        for raw, lo, n, front in self.made:
            assert raw[lo:].data_ptr() % 256 == front, "the view is meant to be off the 256-B grid"
            assert bool((raw[:lo] == GUARD).all()), f"bytes in front of a workspace of {n} B were written"
            assert bool((raw[lo + n:] == GUARD).all()), f"bytes behind a workspace of {n} B were written"
        return len(self.made)


@pytest.fixture
def guarded(monkeypatch):
    """replaces _lib.workspace as described above; the returned Guard checks the guard bytes of every workspace handed out
    since, and answers how many there were"""
    from vdetr_amd import _lib
    guard = Guard()
    monkeypatch.setattr(_lib, "workspace", guard.workspace)
    return guard
