"""nbmf_mm_amd — MI355X-native NBMF-MM (drop-in for ``nbmf_mm``'s NumPy path).

Export list mirrors src/nbmf_mm/__init__.py:10-17 of the reference; ``PackedBits`` (bit-packed binary input) and
``holdout_mask`` (the entries ``fit(holdout=...)`` holds out) are extensions.
"""
from ._base import NBMF, NBMFMM, holdout_mask
from ._metrics import Moments
from ._packed import PackedBits
from ._solver import nbmf_mm_solver

__version__ = "0.1.0"
# (``PackedBits``, ``holdout_mask`` and ``Moments`` (what ``NBMF.expected_counts`` returns) are importable from here but stay out of ``__all__``: the star-import surface is the reference's)
__all__ = ["NBMFMM", "NBMF", "nbmf_mm_solver"]
