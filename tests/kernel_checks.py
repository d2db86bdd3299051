"""Helpers shared by the per-kernel GPU tests (test_gpu_train_kernels.py, test_gpu_kernel_builds.py): run twice and require the
same bits, bound an error a priori, or hold it against a yardstick (the same computation in torch fp32 on the CPU); the worst
ratios go to the agreement records <prefix>_<kernel> (conftest.record_agreement)."""
import torch

from conftest import record_agreement

D, F32, I32 = torch.float64, torch.float32, torch.int32
U = 2.0 ** -24          # fp32 unit roundoff
TINY = 1e-30


def same_bits(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    if a.dtype == F32:
        a, b = a.view(I32), b.view(I32)
    elif a.dtype == D:
        a, b = a.view(torch.int64), b.view(torch.int64)
    return a.shape == b.shape and torch.equal(a, b)


def exact(a, b):
    """Equal values (a zero's sign aside: the kernels' sums start from +0); the inputs hold no NaN."""
    return a.shape == b.shape and torch.equal(a.detach().cpu(), b.detach().cpu())


def _tensors(r):
    if isinstance(r, dict):
        return [r[k] for k in sorted(r)]
    return list(r) if isinstance(r, (tuple, list)) else [r]


def twice(fn):
    """fn() run twice on the same inputs: every tensor it returns (also inside one level of tuple / list / dict) must repeat
    bit for bit."""
    r1, r2 = fn(), fn()
    for x, y in zip(_tensors(r1), _tensors(r2)):
        for u, v in zip(_tensors(x), _tensors(y)):
            if isinstance(u, torch.Tensor):
                assert same_bits(u, v), "two runs on the same inputs differ"
    return r1


class Recorder:
    """The worst measured ratios per kernel, written to the agreement record ``<prefix>_<kernel>`` as they grow."""

    def __init__(self, prefix):
        self.prefix, self.worst = prefix, {}

    def note(self, kernel, **kv):
        w = self.worst.setdefault(kernel, {})
        for k, v in kv.items():
            w[k] = max(w.get(k, 0.0), float(v))
        record_agreement(f"{self.prefix}_{kernel}", w)

    def bounded(self, kernel, what, got, ref, bound):
        """|got - ref| <= bound elementwise (ref fp64); records the worst error / bound."""
        err = (got.detach().cpu().double() - ref).abs()
        ratio = float((err / bound).max()) if err.numel() else 0.0
        self.note(kernel, **{f"{what}_err_over_bound": ratio, "max_abs_err_vs_fp64": float(err.max()) if err.numel() else 0.0})
        assert ratio <= 1.0, f"{kernel} {what}: error {float(err.max()):.3e} beyond the bound (ratio {ratio:.2f})"

    def yardstick(self, kernel, what, got, ref64, ref32, floor_rel=2e-6, factor=4.0):
        """max |got - ref64| <= factor * max |ref32 - ref64| + floor_rel * max |ref64|: the kernel's error within a few times that
        of torch's own fp32 computation on the CPU (plus a floor for where that happens to be exact)."""
        got = got.detach().cpu().double()
        scale = float(ref64.abs().max()) if ref64.numel() else 0.0
        ek = float((got - ref64).abs().max()) if ref64.numel() else 0.0
        ey = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
        floor = floor_rel * scale + TINY
        self.note(kernel, **{f"{what}_yardstick_ratio": ek / (ey + floor), "max_rel_err_vs_fp64": ek / (scale + TINY)})
        assert ek <= factor * ey + floor, f"{kernel} {what}: error {ek:.3e} vs fp32 yardstick {ey:.3e} (scale {scale:.3e})"
