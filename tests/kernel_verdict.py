"""TEST INFRASTRUCTURE ONLY -- the verdict of the per-kernel tests, shared by tests/transolver_kernel_cases.py and
tests/mwt_kernel_cases.py (a plain helper module: no conftest, no fixture).  The two measures and the conditioning cap are those of
tests/unet_kernel_cases.py."""
from unet_kernel_cases import BADLY_CONDITIONED, MEASURES, measures          # noqa: F401


def bound_of(e32, floor=1e-6):
    """what a kernel may be off by where the fp32 restatement is off by ``e32``: 8 times that, and never less than ``floor``"""
    return max(8 * e32, floor)


def verdict(tag, name, figures, existing=None, floor=1e-6):
    """``figures``: (measure, e32, kernel error) triples; the bound is ``bound_of(e32, floor)``, or ``existing`` (a bound another test of
    the same kernel already asserts) INSTEAD of it.  Every figure is printed before the first assertion; a case whose fp32 restatement
    is itself off by more than the cap / 8 is rejected as badly conditioned.  The kernel's error never enters a bound."""
    rows = []
    for kind, e32, ek in figures:
        bound = existing if existing is not None else bound_of(e32, floor)
        print(f"[{tag}] {name} {kind}: e32 {e32:.3e} kernel {ek:.3e} bound {bound:.3e}")
        rows.append((kind, e32, ek, bound))
    for kind, e32, ek, bound in rows:
        assert 8 * e32 <= BADLY_CONDITIONED, f"{name}: badly conditioned inputs, the fp32 restatement itself is off by {e32:.3e} ({kind})"
        assert ek <= bound, f"{name} {kind}: kernel error {ek:.3e} > {bound:.3e} (fp32 restatement: {e32:.3e})"
