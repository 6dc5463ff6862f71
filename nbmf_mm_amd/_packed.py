"""Bit-packed binary matrices: one bit per entry on the host and across PCIe, unpacked on the device.

The layout is NumPy's own: a matrix of logical shape ``(rows, n)`` is the uint8 array ``np.packbits(A != 0, axis=1)`` of
shape ``(rows, ceil(n / 8))`` -- every row packed on its own, entry ``j`` of a row in bit ``7 - j % 8`` of its byte
``j // 8``.  The pad bits of a row's last byte mean nothing and may hold anything.
"""
from __future__ import annotations

import numpy as np


class PackedBits:
    """A binary matrix (data, a mask, an exclude matrix) held as bits.

    ``bits``: a 2-D uint8 array with ``shape[0]`` rows of at least ``ceil(n / 8)`` bytes, unit stride along a row and a
    row stride of at least ``ceil(n / 8)`` bytes -- a row slice of a wider packed array is taken as it is, nothing is
    copied; bytes of a row beyond ``ceil(n / 8) - 1`` are never read.  ``shape``: the logical ``(rows, n)``.

    Wherever the estimator and the solver take a dense bool matrix they take a ``PackedBits``, with the same result bit
    for bit.  What it offers itself is small on purpose: ``shape``, ``nbytes``, ``toarray()``, ``at(rows, cols)``, and row
    slices ``P[r0:r1]`` (step 1).  Anything else -- a column slice, ``.T``, arithmetic -- is not there: unpack with
    ``toarray()`` first.
    """

    ndim = 2
    #: NumPy leaves binary operators with an ndarray to this class instead of iterating over it
    __array_ufunc__ = None

    def __init__(self, bits, shape):
        if isinstance(bits, PackedBits):
            raise TypeError("bits must be a uint8 array, not a PackedBits")
        bits = np.asarray(bits)
        if bits.dtype != np.uint8:
            raise TypeError(f"bits must be a uint8 array (got dtype {bits.dtype})")
        if bits.ndim != 2:
            raise ValueError(f"bits must be 2-D (got shape {bits.shape})")
        try:
            rows, n = shape
            rows, n = int(rows), int(n)
        except (TypeError, ValueError):
            raise ValueError(f"shape must be (rows, n) (got {shape!r})") from None
        if rows < 0 or n < 0:
            raise ValueError(f"shape must be non-negative (got {(rows, n)})")
        nb = (n + 7) // 8
        if bits.shape[0] != rows or bits.shape[1] < nb:
            raise ValueError(f"a packed {rows} x {n} matrix is {rows} rows of at least {nb} bytes (got bits of shape {bits.shape})")
        bits = bits[:, :nb]                               # (a view: the bytes that are read)
        if bits.size and ((nb > 1 and bits.strides[1] != 1) or (rows > 1 and bits.strides[0] < nb)):
            raise ValueError("bits must have unit stride along a row and a row stride of at least ceil(n / 8) bytes")
        self.bits = bits
        self.shape = (rows, n)

    @classmethod
    def from_dense(cls, A):
        """Pack ``A != 0`` of a dense 2-D array of any dtype."""
        A = np.asarray(A)
        if A.ndim != 2:
            raise ValueError(f"a 2-D array is expected (got shape {A.shape})")
        return cls(np.packbits(A != 0, axis=1), A.shape)

    @property
    def nbytes(self):
        """The bytes the packed rows occupy: ``rows * ceil(n / 8)``."""
        return self.shape[0] * ((self.shape[1] + 7) // 8)

    @property
    def ld(self):
        """The row stride in bytes as the library takes it (of a single row or an empty matrix: ``ceil(n / 8)``)."""
        return int(self.bits.strides[0]) if self.bits.size and self.shape[0] > 1 else (self.shape[1] + 7) // 8

    @property
    def T(self):
        raise ValueError("a PackedBits cannot be transposed: rows are packed on their own (use toarray())")

    def __len__(self):
        return self.shape[0]

    def __repr__(self):
        return f"PackedBits(shape={self.shape}, nbytes={self.nbytes})"

    def toarray(self):
        """The dense bool matrix."""
        rows, n = self.shape
        if n == 0:
            return np.zeros((rows, 0), dtype=np.bool_)
        return np.unpackbits(self.bits, axis=1, count=n).view(np.bool_)

    def at(self, rows, cols):
        """The entries at the index pairs ``(rows[t], cols[t])`` as a bool array."""
        rows, cols = np.asarray(rows), np.asarray(cols)
        for name, a in (("rows", rows), ("cols", cols)):
            if not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{name} must be an integer array (got dtype {a.dtype})")
        if rows.shape != cols.shape:
            raise ValueError(f"rows and cols must have the same shape (got {rows.shape} and {cols.shape})")
        if rows.size and (rows.min() < 0 or rows.max() >= self.shape[0] or cols.min() < 0 or cols.max() >= self.shape[1]):
            raise ValueError(f"an index pair is outside the {self.shape[0]} x {self.shape[1]} matrix")
        return ((self.bits[rows, cols >> 3] >> (7 - (cols & 7)).astype(np.uint8)) & 1).astype(np.bool_)

    def __getitem__(self, key):
        if not isinstance(key, slice):
            raise TypeError("a PackedBits takes row slices P[r0:r1] only (use toarray() or at() for anything else)")
        r0, r1, step = key.indices(self.shape[0])
        if step != 1:
            raise ValueError("a PackedBits takes row slices with step 1 only")
        r1 = max(r0, r1)
        return PackedBits(self.bits[r0:r1], (r1 - r0, self.shape[1]))
