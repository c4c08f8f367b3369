"""The guard fixture of tests/workspace_guard.py on itself: torch only, no kernel of the project, no GPU.  A byte written one past
the view, or one in front of it, fails the check; bytes written inside the view do not; the view is off the 256-B grid by the
offset asked for, poisoned with 0xFF, and the tail guard holds one whole unit of the layout."""
import pytest
import torch

from workspace_guard import GUARD, POISON, guarded  # noqa: F401


@pytest.mark.parametrize("front,unit,n", [(8, 0, 100), (16, 0, 96), (16, 4096, 1000), (8, 300, 1)])
def test_guard_sees_a_byte_on_either_side(guarded, front, unit, n):
    from vdetr_amd import _lib
    guarded.layout(front=front, unit=unit)
    ws = _lib.workspace(n, "cpu")
    assert ws.dtype == torch.uint8 and ws.numel() == n and ws.data_ptr() % 256 == front
    assert bool((ws == POISON).all())
    blk = guarded.block(0)
    assert blk.data_ptr() % 256 == 0 and blk.numel() >= front + n + max(256, unit)
    assert bool((blk[:front] == GUARD).all()) and bool((blk[front + n:] == GUARD).all())
    assert guarded() == 1
    ws.zero_()  # every byte of the view itself belongs to the op
    assert guarded() == 1 and bool((guarded.interior(0) == 0).all())
    blk[front + n] = 0
    with pytest.raises(AssertionError, match=f"behind a workspace of {n} B"):
        guarded()
    blk[front + n] = GUARD
    assert guarded() == 1
    blk[front + n + max(256, unit) - 1] = 0  # the last byte of one further unit
    with pytest.raises(AssertionError, match="behind a workspace"):
        guarded()
    blk[front + n + max(256, unit) - 1] = GUARD
    blk[front - 1] = 0
    with pytest.raises(AssertionError, match=f"in front of a workspace of {n} B"):
        guarded()
    blk[front - 1] = GUARD
    assert guarded() == 1


def test_guard_counts_and_keeps_each_workspaces_own_layout(guarded):
    from vdetr_amd import _lib
    a = _lib.workspace(0, "cpu")  # (a request of nothing is one byte, as _lib.workspace gives)
    guarded.layout(front=16, unit=1024)
    b = _lib.workspace(40, "cpu")
    assert a.numel() == 1 and a.data_ptr() % 256 == 8 and b.data_ptr() % 256 == 16
    assert guarded() == 2
    guarded.block(1)[16 + 40 + 1023] = 1
    with pytest.raises(AssertionError, match="behind a workspace of 40 B"):
        guarded()


def test_layout_refuses_a_front_that_breaks_a_contract(guarded):
    with pytest.raises(AssertionError):
        guarded.layout(front=4)
    with pytest.raises(AssertionError):
        guarded.layout(front=256)
