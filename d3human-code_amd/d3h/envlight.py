"""Host side of csrc/envlight.hip: the sampling tables of a lat-long environment light (render/light.py:46-59, EnvironmentLight.update_pdf).

tables(base [H,W,3]) -> (pdf [H,W], rows [H,W], cols [H,W]), float32, no gradient (the reference computes them under torch.no_grad()).  `rows` is the
[H] table expanded along W without a copy: the reference keeps the repeated [H,W] shape and its callers read `rows[:, 0]`.  Two launches, no atomics,
no synchronisation; the tables are exactly non-decreasing and end in exactly 1 (csrc/envlight.hip says why that needs care)."""
import torch

from . import _lib as L


def tables(base):
    if base.dim() != 3 or base.shape[-1] != 3 or base.shape[0] < 1 or base.shape[1] < 1:
        raise RuntimeError(f'envlight.tables: expected base [H,W,3] with H, W >= 1, got {tuple(base.shape)}')
    H, W = int(base.shape[0]), int(base.shape[1])
    base = base.detach().float().contiguous()
    pdf, cols = (torch.empty(H, W, dtype=torch.float32, device=base.device) for _ in range(2))
    rows, rowtot = (torch.empty(H, dtype=torch.float32, device=base.device) for _ in range(2))
    L.call('envlight_tables', base, H, W, pdf, rows, cols, rowtot)
    return pdf, rows[:, None].expand(H, W), cols
