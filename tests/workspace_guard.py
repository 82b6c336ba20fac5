"""Guarded workspaces for the C-ABI overrun tests: exactly the bytes a *_workspace_size
function returned, filled with a chosen byte, and a guard of 0x5A behind them that a call
writing past its workspace would disturb."""
import torch

GUARD = 4096


def guarded(nbytes, fill, device="cuda"):
    ws = torch.empty(nbytes + GUARD, dtype=torch.uint8, device=device)
    ws[:nbytes] = fill
    ws[nbytes:] = 0x5A
    return ws


def guard_intact(ws, nbytes):
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0x5A).all(), "the call wrote past the workspace it asked for"
