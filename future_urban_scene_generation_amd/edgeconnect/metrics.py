"""Drop-in for the reference's ``edgeconnect.metrics``: ``PSNR(max_val)`` and ``EdgeAccuracy(threshold=0.5)`` with the same
constructor arguments, call signatures and return conventions (whole-tensor 0-d tensors).

On HIP tensors the counting and the sum of squared differences run on the device (ops.edge_counts, ops.image_metrics_u8,
ops.sq_diff_sum) and ONE small read-back brings the integers / the float64 sum to the host, where the few scalar steps are
done in float64 - the reference's own `if relevant == 0` / `if mse == 0` wait for the device just the same.  On CPU tensors
the host twins of the same kernels (or plain torch in float64) are used; no device is needed.  The results are float32
tensors like the reference's, computed from exact counts instead of float32 sums."""
import math

import torch
import torch.nn as nn

FUSG_DROPIN = True


def _as_rows(t: torch.Tensor) -> torch.Tensor:
    """Any tensor as float32 [rows, 1, H, W] (what the counting kernel takes)."""
    t = t.to(torch.float32)
    if t.dim() == 4 and t.shape[1] == 1:
        return t
    if t.dim() >= 2:
        return t.reshape(-1, 1, t.shape[-2], t.shape[-1])
    return t.reshape(1, 1, 1, -1)


def _edge_totals(x: torch.Tensor, y: torch.Tensor, threshold: float):
    """(relevant, selected, true positives) over the whole tensors, as Python ints."""
    from .. import ops
    if x.shape != y.shape:
        raise ValueError(f"EdgeAccuracy: shapes {tuple(x.shape)} and {tuple(y.shape)} differ")
    x, y = _as_rows(x), _as_rows(y)
    if x.is_cuda:
        counts = ops.d2h(ops.edge_counts(x, y.to(x.device), threshold))
    else:
        counts = ops.edge_counts_host(x.numpy(), y.numpy(), threshold)
    rel, sel, tp = (int(v) for v in counts.sum(axis=0))
    return rel, sel, tp


class EdgeAccuracy(nn.Module):
    """Precision and recall of an edge map against its labels, both thresholded with a strict `>`."""

    def __init__(self, threshold=0.5):
        super().__init__()
        self.threshold = threshold

    def __call__(self, inputs, outputs):
        relevant, selected, true_positive = _edge_totals(inputs, outputs, self.threshold)
        if relevant == 0 and selected == 0:
            return torch.tensor(1), torch.tensor(1)
        precision = true_positive / (selected + 1e-8)
        recall = true_positive / (relevant + 1e-8)
        dev = inputs.device
        return torch.tensor(precision, dtype=torch.float32, device=dev), torch.tensor(recall, dtype=torch.float32, device=dev)


def _fits_table(a: torch.Tensor, b: torch.Tensor) -> bool:
    """A uint8 [B, H, W, C] pair the metrics table takes."""
    return (a.dtype == torch.uint8 and b.dtype == torch.uint8 and a.dim() == 4 and a.shape == b.shape and 1 <= a.shape[3] <= 4
            and 11 <= a.shape[1] < 32768 and 11 <= a.shape[2] < 32768 and a.shape[0] < 65536)


def _sse(a: torch.Tensor, b: torch.Tensor) -> float:
    """sum((a - b)^2) over the whole tensors, in float64."""
    from .. import ops
    if a.shape != b.shape:
        raise ValueError(f"PSNR: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    col = ops.IMAGE_METRIC_COLUMNS.index("sse")
    if a.is_cuda:
        if _fits_table(a, b):
            return float(ops.d2h(ops.image_metrics_u8(a, b.to(a.device))[:, col]).sum())
        return float(ops.d2h(ops.sq_diff_sum(a, b.to(a.device))))
    if _fits_table(a, b):
        return float(ops.image_metrics_host(a.numpy(), b.numpy())[:, col].sum())
    return float(((a.double() - b.double()) ** 2).sum())


class PSNR(nn.Module):
    """Peak signal-to-noise ratio in dB, 20 log10(max_val) - 10 log10(mse); 0 when the two tensors are equal."""

    def __init__(self, max_val):
        super().__init__()
        self.register_buffer("base10", torch.log(torch.tensor(10.0)))
        self.register_buffer("max_val", torch.tensor(20.0 * math.log10(float(max_val)), dtype=torch.float32))
        self._peak_db = 20.0 * math.log10(float(max_val))

    def __call__(self, a, b):
        n = a.numel()
        mse = _sse(a, b) / n if n else float("nan")
        if mse == 0:
            return torch.tensor(0)
        return torch.tensor(self._peak_db - 10.0 * math.log10(mse), dtype=torch.float32, device=a.device)
