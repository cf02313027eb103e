"""Matrix / TransposedMatrix: the host-side mirror of graphblas/core/matrix.py for the path --
constructor :190-203, ``__del__`` :218-225, ``build`` :627-681, ``from_coo`` :818-894, ``_from_csx``
:992-1068, ``to_coo`` :525-594, ``_to_csx`` :1601-1645, ``isequal`` :373-415, ``ewise_add`` :1861-1950,
``ewise_mult`` :1952-2041, ``mxv`` :2203-2262, ``mxm`` :2264-2331, ``__getitem__`` :3020-3090, ``TransposedMatrix`` :3900-3960."""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .base import BaseType, Expression, InfixMatMul, Mask, ScalarExpression, apply_expression, call, call_on, select_expression
from .descriptor import lookup as descriptor_lookup
from .dtypes import lookup_dtype
from .exceptions import DimensionMismatch
from .operators import binary as _binary, get_typed_op, monoid as _monoid, semiring as _semiring
from .vector import Vector, _iptr, _name_counter, _ptr

GrB_CSR_FORMAT, GrB_CSC_FORMAT = 0, 1


def _cast_scalar(value, np_type):
    """The GraphBLAS typecast of ONE host number, as the library casts an entry (cast_value, csrc/grb_ops.hpp): to BOOL ``x != 0``;
    floating point -> integer truncates and saturates, NaN -> 0; integer -> integer wraps.  (numpy's own conversion of 300.7 or NaN to
    an integer type is undefined, and of an integer beyond the type's range an error.)"""
    np_type = np.dtype(np_type)
    v = np.asarray(value)
    if np_type.kind == "b":
        return np.bool_(bool(v != 0))
    if np_type.kind not in "iu":
        with np.errstate(over="ignore"):
            return np_type.type(value)
    info = np.iinfo(np_type)
    if v.dtype.kind == "f":
        x = float(v)
        q = 0 if x != x else (int(info.min) if x <= float(info.min) else (int(info.max) if x >= float(info.max) else int(x)))
    else:
        q = int(v) % (1 << info.bits)
        q -= (1 << info.bits) if q > info.max else 0
    return np_type.type(q)


def _owned_copy(arr):
    """A malloc'd copy of a numpy array: the GxB import / pack entries take OWNERSHIP of their host arrays and release them with
    the library's deallocator (the reference hands over numpy buffers it has unclaimed, core/ss/matrix.py:1300-1349)."""
    libc = ctypes.CDLL(None)
    libc.malloc.restype = ctypes.c_void_p
    libc.malloc.argtypes = [ctypes.c_size_t]
    nbytes = max(int(arr.nbytes), 1)
    p = libc.malloc(nbytes)
    if not p:
        raise MemoryError
    if arr.nbytes:
        ctypes.memmove(p, arr.ctypes.data, arr.nbytes)
    return ctypes.c_void_p(p), int(arr.nbytes)


class _MatrixSS:
    """``Matrix.ss`` / ``A.ss``: the reference's SuiteSparse namespace (graphblas/core/ss/matrix.py), reduced to the ingress the
    hot path's callers use -- ``import_csr`` (:1139-1237) and ``pack_csr`` (:1239-1277), both through ``_import_csr``
    (:1279-1349) -> ``GxB_Matrix_{import,pack}_CSR``.  Same keyword arguments; ``take_ownership`` is accepted and means nothing
    here (the matrix lives in HBM: the host arrays are copied once either way, and the caller's numpy arrays are left alone).
    On an instance -- also on ``A.T`` -- ``sort`` (:3983-4048 -> ``GxB_Matrix_sort``) and the ``compactify`` by value (:3869-3981) built on it."""

    def __init__(self, parent=None):
        self._parent = parent

    @staticmethod
    def _csr_args(indptr, values, col_indices, dtype, is_iso, fmt):
        if fmt is not None and fmt.lower() != "csr":
            raise ValueError(f"Invalid format: {fmt!r}.  Must be None or 'csr'.")
        indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
        col_indices = np.ascontiguousarray(col_indices, dtype=np.uint64)
        values = np.asarray(values)
        dtype = lookup_dtype(dtype if dtype is not None else values.dtype)
        values = np.ascontiguousarray(np.atleast_1d(values).astype(dtype.np_type, copy=False))
        if is_iso:
            values = values[:1]
        ptrs = [_owned_copy(a) for a in (indptr, col_indices, values)]
        cells = [ctypes.c_void_p(p.value) for p, _ in ptrs]
        return dtype, cells, [nb for _, nb in ptrs]

    @staticmethod
    def _release_leftovers(cells):
        libc = ctypes.CDLL(None)
        libc.free.argtypes = [ctypes.c_void_p]
        for c in cells:  # (a failed call leaves the arrays with the caller: *Ap & co. are still set)
            if c.value:
                libc.free(c)

    def import_csr(self, *, nrows, ncols, indptr, values, col_indices, is_iso=False, sorted_cols=False, take_ownership=False,
                   dtype=None, format=None, name=None, **opts):
        dtype, cells, sizes = self._csr_args(indptr, values, col_indices, dtype, is_iso, format)
        A = Matrix.__new__(Matrix)
        A.dtype, A._nrows, A._ncols, A.name = dtype, int(nrows), int(ncols), name or f"M_{next(_name_counter)}"
        A._handle = ctypes.c_void_p()
        _lib.load()
        try:
            call_on(None, "GxB_Matrix_import_CSR",
                    [ctypes.byref(A._handle), dtype._carg, A._nrows, A._ncols, ctypes.byref(cells[0]), ctypes.byref(cells[1]),
                     ctypes.byref(cells[2]), sizes[0], sizes[1], sizes[2], bool(is_iso), not sorted_cols, None])
        finally:
            self._release_leftovers(cells)
        return A

    def pack_csr(self, *, indptr, values, col_indices, is_iso=False, sorted_cols=False, take_ownership=False, format=None,
                 nrows=None, ncols=None, dtype=None, name=None, **opts):
        A = self._parent
        if A is None:
            raise TypeError("pack_csr packs into an existing Matrix: call it on an instance (A.ss.pack_csr(...))")
        _dt, cells, sizes = self._csr_args(indptr, values, col_indices, A.dtype, is_iso, format)
        try:
            call_on(A, "GxB_Matrix_pack_CSR",
                    [A._handle, ctypes.byref(cells[0]), ctypes.byref(cells[1]), ctypes.byref(cells[2]), sizes[0], sizes[1], sizes[2],
                     bool(is_iso), not sorted_cols, None])
        finally:
            self._release_leftovers(cells)
        return A

    def sort(self, op=_binary.lt, order="rowwise", *, values=True, permutation=True, nthreads=None, **opts):
        """``C, P = A.ss.sort(op, order)``: the values of every row (``order="columnwise"``: of every column) in the order of ``op`` --
        ``binary.lt`` / ``"<"`` ascending, ``binary.gt`` / ``">"`` descending --, moved to the left (to the top), and the column (row)
        index each value had; both have the shape and ``C`` the dtype of ``A``, ``P`` is UINT64.  Ties go to the smaller index, NaNs
        come last under both operators.  ``values=False`` / ``permutation=False``: that output is ``None`` and is not computed.
        ``nthreads`` is accepted and ignored.  On ``A.T`` the order flips.  (reference core/ss/matrix.py:3983-4048 -> C
        ``GxB_Matrix_sort``)"""
        A = self._require_parent("sort")
        base = A._matrix
        top = sort_operator(op, base.dtype)
        columnwise = (sort_order(order) == "columnwise") != A._is_transposed
        if not values and not permutation:
            return None, None
        descriptor_lookup(**opts)  # (no descriptor option exists beyond the transpose: anything else is the caller's error)
        C = Matrix(base.dtype, A._nrows, A._ncols, name="Values") if values else None
        P = Matrix("UINT64", A._nrows, A._ncols, name="Permutation") if permutation else None
        if A._is_transposed:  # (the sort runs on the stored matrix: its outputs have the stored shape and are turned afterwards)
            Cs = Matrix(base.dtype, base._nrows, base._ncols) if values else None
            Ps = Matrix("UINT64", base._nrows, base._ncols) if permutation else None
        else:
            Cs, Ps = C, P
        desc = descriptor_lookup(transpose_first=columnwise)
        if Cs is not None:
            call("GxB_Matrix_sort", [Cs, Ps, top, base, desc])
        else:
            call_on(Ps, "GxB_Matrix_sort", [None, Ps._carg, top._carg, base._carg, desc._carg if desc is not None else None])
        if A._is_transposed:
            for out, stored in ((C, Cs), (P, Ps)):
                if out is not None:
                    call("GrB_transpose", [out, None, None, stored, None])
        return C, P

    def compactify(self, how="first", k=None, order="rowwise", *, reverse=False, asindex=False, name=None):
        """The ``k`` smallest (``how="smallest"``, ascending) or largest (``"largest"``, descending) values of every row -- column,
        ``order="columnwise"`` -- moved to the left (top), as a new Matrix with ``k`` columns (rows); ``k=None``: as many as the longest
        row holds.  ``reverse``: each row's kept values in reverse order; ``asindex``: the column (row) indices of the values instead
        (UINT64).  Built from :meth:`sort` and ``select("col<=", k - 1)`` on the device (reference core/ss/matrix.py:3869-3981, whose
        ``"first"``, ``"last"`` and ``"random"`` this library does not have)."""
        from .exceptions import NotImplementedException

        A = self._require_parent("compactify")
        how = how.lower()
        if how not in {"first", "last", "smallest", "largest", "random"}:
            raise ValueError('`how` argument must be one of: "first", "last", "smallest", "largest", "random"')
        if how not in {"smallest", "largest"}:
            raise NotImplementedException(f'compactify(how="{how}") is not implemented: "smallest" and "largest" are')
        columnwise = sort_order(order) == "columnwise"
        if k is not None:
            k = int(k)
            if k < 0:
                raise ValueError("k must be non-negative")
        C, P = self.sort(_binary.lt if how == "smallest" else _binary.gt, order, values=not asindex, permutation=asindex)
        X = P if asindex else C
        dim = X._nrows if columnwise else X._ncols
        if k is not None and k < dim:
            X = X.select("row<=" if columnwise else "col<=", k - 1).new()
        if reverse:
            if columnwise:
                Y = X.T.new()
                call("GrX_Matrix_reverse_rows", [Y, Y])
                X = Y.T.new()
            else:
                call("GrX_Matrix_reverse_rows", [X, X])
        if k is None:  # the longest row: the columns of the compacted matrix that hold an entry
            k = (X.reduce_rowwise("any") if columnwise else X.reduce_columnwise("any")).new().nvals
        X.resize(*((k, X._ncols) if columnwise else (X._nrows, k)))
        if name is not None:
            X.name = name
        return X

    def _require_parent(self, what):
        if self._parent is None:
            raise TypeError(f"{what} works on a Matrix instance: A.ss.{what}(...)")
        return self._parent


def sort_order(order):
    """"rowwise" or "columnwise" from the reference's spellings (core/utils.py get_order)."""
    val = order.lower() if isinstance(order, str) else order
    if val in {"c", "col", "cols", "column", "columns", "colwise", "columnwise"}:
        return "columnwise"
    if val in {"r", "row", "rows", "rowwise"}:
        return "rowwise"
    raise ValueError(f"Bad value for order: {order!r}.  Expected 'rowwise', 'columnwise', 'rows', or 'columns', 'row', 'col', 'r', 'c'.")


def sort_operator(op, dtype):
    """The typed binary operator of a sort: a BinaryOp, its string spelling, or a Monoid standing for its binary operator (the way
    ``apply`` takes them).  Which operators sort is the library's answer (GrB_LT / GrB_GT; DomainMismatch, NotImplementedException)."""
    top = get_typed_op(op, dtype, kind="binary")
    if top.opclass == "Monoid":
        top = top.binaryop
    return top


class _SSAccessor:
    def __get__(self, obj, objtype=None):
        return _MatrixSS(obj)


class Matrix(BaseType):
    _grb_kind = "Matrix"
    ndim = 2
    _is_transposed = False
    ss = _SSAccessor()  # Matrix.ss.import_csr(...), A.ss.pack_csr(...): reference core/ss/matrix.py:1139-1349

    def __init__(self, dtype=float, nrows=0, ncols=0, *, name=None):
        self.dtype = lookup_dtype(dtype)
        self._nrows, self._ncols = int(nrows), int(ncols)
        self.name = name or f"M_{next(_name_counter)}"
        self._handle = ctypes.c_void_p()
        _lib.load()
        call_on(None, "GrB_Matrix_new", [ctypes.byref(self._handle), self.dtype._carg, self._nrows, self._ncols])

    @property
    def _carg(self):
        return self._handle

    @property
    def _matrix(self):
        return self

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value and _lib is not None and _lib.lib is not None:
            try:
                _lib.lib.GrB_Matrix_free(ctypes.byref(h))
            except Exception:  # interpreter shutdown
                pass

    nrows = property(lambda self: self._nrows)
    ncols = property(lambda self: self._ncols)
    shape = property(lambda self: (self._nrows, self._ncols))

    @property
    def nvals(self):
        n = ctypes.c_uint64()
        call_on(self, "GrB_Matrix_nvals", [ctypes.byref(n), self._handle])
        return int(n.value)

    @property
    def T(self):
        return TransposedMatrix(self)

    def __repr__(self):
        return f"Matrix<{self.dtype}, {self._nrows}x{self._ncols}, name={self.name}>"

    # ---- ingress / egress ---------------------------------------------------------------------------------
    def build(self, rows, columns, values, *, dup_op=None, clear=False):
        """reference core/matrix.py:627-681: uint64 indices (:637-638), default dup_op=plus with
        duplicate detection by nvals < n (:657-681)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        columns = np.ascontiguousarray(columns, dtype=np.uint64)
        values = np.asarray(values)
        if values.ndim == 0:
            values = np.broadcast_to(values, rows.shape)
        values = np.ascontiguousarray(values.astype(self.dtype.np_type, copy=False))
        n = values.size
        if rows.size != n or columns.size != n:
            raise ValueError(f"`rows` and `columns` and `values` lengths must match: {rows.size}, {columns.size}, {n}")
        if clear:
            self.clear()
        if n == 0:
            return
        dup_orig = dup_op
        if dup_op is None:
            dup_op = "plus"
        dup_t = get_typed_op(dup_op, self.dtype, kind="binary")
        if dup_t.opclass == "Monoid":
            dup_t = dup_t.binaryop
        call(f"GrB_Matrix_build_{self.dtype.name}", [self, _ptr(rows), _ptr(columns), _ptr(values), n, dup_t])
        if dup_orig is None and self.nvals < n:
            self.clear()
            raise ValueError("Duplicate indices found, must provide `dup_op` BinaryOp")

    @classmethod
    def from_coo(cls, rows, columns, values=1.0, dtype=None, *, nrows=None, ncols=None, dup_op=None, name=None):
        """reference core/matrix.py:818-894: shape inferred as max index + 1 when not given."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        columns = np.ascontiguousarray(columns, dtype=np.uint64)
        values = np.asarray(values)
        if dtype is None:
            dtype = lookup_dtype(values.dtype) if values.dtype.kind in "biuf" else lookup_dtype(float)
        if nrows is None:
            if rows.size == 0:
                raise ValueError("No row indices provided. Unable to infer nrows.")
            nrows = int(rows.max()) + 1
        if ncols is None:
            if columns.size == 0:
                raise ValueError("No column indices provided. Unable to infer ncols.")
            ncols = int(columns.max()) + 1
        C = cls(dtype, nrows, ncols, name=name)
        C.build(rows, columns, values, dup_op=dup_op)
        return C

    @classmethod
    def _from_csx(cls, fmt, indptr, indices, values, dtype, num, name):
        indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
        indices = np.ascontiguousarray(indices, dtype=np.uint64)
        values = np.asarray(values)
        if dtype is None:
            dtype = lookup_dtype(values.dtype)
        dtype = lookup_dtype(dtype)
        if values.ndim == 0:
            values = np.broadcast_to(values, indices.shape)
        values = np.ascontiguousarray(values.astype(dtype.np_type, copy=False))
        if num is None:
            num = int(indices.max()) + 1 if indices.size else 0
        nrows, ncols = (indptr.size - 1, num) if fmt == GrB_CSR_FORMAT else (num, indptr.size - 1)
        A = cls.__new__(cls)
        A.dtype, A._nrows, A._ncols, A.name = dtype, nrows, ncols, name or f"M_{next(_name_counter)}"
        A._handle = ctypes.c_void_p()
        _lib.load()
        call_on(None, f"GrB_Matrix_import_{dtype.name}",
                [ctypes.byref(A._handle), dtype._carg, nrows, ncols, _ptr(indptr), _ptr(indices), _ptr(values),
                 indptr.size, indices.size, values.size, fmt])
        return A

    @classmethod
    def from_csr(cls, indptr, col_indices, values=1.0, dtype=None, *, ncols=None, name=None):
        return cls._from_csx(GrB_CSR_FORMAT, indptr, col_indices, values, dtype, ncols, name)

    @classmethod
    def from_csc(cls, indptr, row_indices, values=1.0, dtype=None, *, nrows=None, name=None):
        return cls._from_csx(GrB_CSC_FORMAT, indptr, row_indices, values, dtype, nrows, name)

    def to_coo(self, dtype=None, *, rows=True, columns=True, values=True, sort=True):
        """reference core/matrix.py:525-594 (row-major sorted)."""
        n = self.nvals
        I = np.empty(n, np.uint64) if rows else None
        J = np.empty(n, np.uint64) if columns else None
        X = np.empty(n, self.dtype.np_type) if values else None
        cnt = ctypes.c_uint64(n)
        call_on(self, f"GrB_Matrix_extractTuples_{self.dtype.name}",
                [_ptr(I) if n else None, _ptr(J) if n else None, _ptr(X) if n else None, ctypes.byref(cnt), self._handle])
        if X is not None and dtype is not None:
            X = X.astype(lookup_dtype(dtype).np_type)
        return I, J, X

    def _to_csx(self, fmt):
        ap, ai, ax = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        call_on(self, "GrB_Matrix_exportSize", [ctypes.byref(ap), ctypes.byref(ai), ctypes.byref(ax), fmt, self._handle])
        Ap = np.empty(ap.value, np.uint64)
        Ai = np.empty(ai.value, np.uint64)
        Ax = np.empty(ax.value, self.dtype.np_type)
        call_on(self, f"GrB_Matrix_export_{self.dtype.name}",
                [_ptr(Ap), Ai.ctypes.data_as(ctypes.c_void_p), Ax.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ap),
                 ctypes.byref(ai), ctypes.byref(ax), fmt, self._handle])
        return Ap[: ap.value], Ai[: ai.value], Ax[: ax.value]

    def to_csr(self):
        return self._to_csx(GrB_CSR_FORMAT)

    def to_csc(self):
        return self._to_csx(GrB_CSC_FORMAT)

    def dup(self, dtype=None, *, clear=False, mask=None, name=None):
        """A copy; ``dtype``: with the values cast (on the device); ``clear``: same shape and dtype, no entries; ``mask``: only the
        entries the mask lets through (reference core/matrix.py:469-497; tests/test_matrix.py:66-96)."""
        dt = self.dtype if dtype is None else lookup_dtype(dtype)
        if clear:
            return Matrix(dt, self._nrows, self._ncols, name=name)
        if mask is not None:
            C = Matrix(dt, self._nrows, self._ncols, name=name)
            C(mask=mask) << self
            return C
        C = Matrix.__new__(Matrix)
        C.dtype, C._nrows, C._ncols, C.name = dt, self._nrows, self._ncols, name or f"M_{next(_name_counter)}"
        C._handle = ctypes.c_void_p()
        if dt is self.dtype:
            call_on(self, "GrB_Matrix_dup", [ctypes.byref(C._handle), self._handle])
        else:  # the typecast copy is made on the device
            call_on(self, "GrX_Matrix_dup_as", [ctypes.byref(C._handle), dt._carg, self._handle])
        return C

    def clear(self):
        call("GrB_Matrix_clear", [self])

    def resize(self, nrows, ncols):
        """In place: growing adds empty rows / columns, shrinking drops the entries beyond the new bounds
        (reference core/matrix.py:512-523)."""
        nrows, ncols = int(nrows), int(ncols)
        if nrows < 0 or ncols < 0:
            raise ValueError("nrows and ncols must be non-negative")
        call("GrB_Matrix_resize", [self, nrows, ncols])
        self._nrows, self._ncols = nrows, ncols

    def isequal(self, other, *, check_dtype=False):
        """Same shape, structure and values (reference core/matrix.py:373-415)."""
        if not isinstance(other, Matrix):
            raise TypeError(f"Expected type: Matrix; got {type(other).__name__}")
        if check_dtype and self.dtype is not other.dtype:
            return False
        if self.shape != other.shape or self.nvals != other.nvals:
            return False
        return self._compare_on_device(other, 0.0, 0.0)

    def _compare_on_device(self, other, rel_tol, abs_tol):
        """pattern and values compared by the library on the device: only the verdict comes back"""
        eq = ctypes.c_bool(False)
        call_on(self, "GrX_Matrix_isclose", [ctypes.byref(eq), self._handle, other._handle, ctypes.c_double(rel_tol), ctypes.c_double(abs_tol)])
        return bool(eq.value)

    def isclose(self, other, *, rel_tol=1e-7, abs_tol=0.0, check_dtype=False):
        if check_dtype and self.dtype is not other.dtype:
            return False
        if self.shape != other.shape or self.nvals != other.nvals:
            return False
        return self._compare_on_device(other, float(rel_tol), float(abs_tol))

    # ---- the hot path ---------------------------------------------------------------------------------------
    def mxv(self, other, op=_semiring.plus_times):
        """``w << A.mxv(v, semiring)``  (reference core/matrix.py:2203-2262 -> C ``GrB_mxv``)."""
        return _mxv(self, other, op)

    def mxm(self, other, op=_semiring.plus_times):
        """``C << A.mxm(B, semiring)``  (reference core/matrix.py:2264-2331 -> C ``GrB_mxm``)."""
        return _mxm(self, other, op)

    def ewise_add(self, other, op=_monoid.plus):
        """``C << A.ewise_add(B, op)``: union of the patterns; ``op`` where both have an entry (reference core/matrix.py
        ewise_add -> C ``GrB_Matrix_eWiseAdd_<opclass>``)."""
        return _ewise(self, other, op, "ewise_add", "GrB_Matrix_eWiseAdd")

    def ewise_mult(self, other, op=_binary.times):
        """``C << A.ewise_mult(B, op)``: intersection of the patterns (reference core/matrix.py ewise_mult -> C
        ``GrB_Matrix_eWiseMult_<opclass>``)."""
        return _ewise(self, other, op, "ewise_mult", "GrB_Matrix_eWiseMult")

    def ewise_union(self, other, op, left_default, right_default):
        """``C << A.ewise_union(B, op, left_default, right_default)``: union of the patterns; ``op(a, b)`` where both have an entry,
        ``op(a, right_default)`` where only A has one, ``op(left_default, b)`` where only B has one -- sparse subtraction is
        ``A.ewise_union(B, binary.minus, 0, 0)`` (reference core/matrix.py:2043-2200 -> C ``GxB_Matrix_eWiseUnion``).  Both defaults are
        required; how they type the operator: :func:`graphblas_amd.base.union_expression`."""
        return _ewise_union(self, other, op, left_default, right_default)

    def diag(self, k=0, dtype=None, *, name=None):
        """The k-th diagonal as a new Vector: ``v[i] = A[i, i + k]`` for ``k >= 0``, ``A[i - k, i]`` for ``k < 0``; ``dtype``: the values
        cast on the device (reference core/matrix.py diag -> C ``GxB_Vector_diag``).  ``k`` may be an int or a Scalar."""
        return _diag_vector(self, k, dtype, name)

    def kronecker(self, other, op=_binary.times):
        """``C << A.kronecker(B, op)``: the Kronecker product, ``C[ia*mb + ib, ja*nb + jb] = op(A[ia, ja], B[ib, jb])`` (reference
        core/matrix.py:2333-2373 -> C ``GrB_Matrix_kronecker_<opclass>``)."""
        return _kronecker(self, other, op)

    def reduce_rowwise(self, op="plus"):
        return _reduce_vector(self, op, "reduce_rowwise", False)

    def reduce_columnwise(self, op="plus"):
        return _reduce_vector(self, op, "reduce_columnwise", True)

    def reduce_scalar(self, op="plus", *, allow_empty=True):
        """``s << A.reduce_scalar(monoid)`` (reference core/matrix.py:2712-2770): here the row reduction on the pull SpMV path
        followed by the vector reduction -- Matrix -> Vector -> Scalar, as the reference's aggregators do (core/operator/agg.py:
        304-330); ``agg.count`` / ``agg.exists`` are the number of entries / whether there is one."""
        return _reduce_scalar(self, op, allow_empty)

    def power(self, n, op=_semiring.plus_times):
        """``C << A.power(n, semiring)`` by repeated squaring (reference core/matrix.py:2840-2905)."""
        return _matrix_power(self, n, op)

    def select(self, op, thunk=None):
        """``C << A.select("tril", -1)`` / ``A.select(">=", 3)`` / ``A.select(M.S)``: the entries the index-unary operator (or the
        mask) keeps (reference core/matrix.py:2597-2623 -> C ``GrB_Matrix_select_<T>``)."""
        return select_expression(self, op, thunk, output_type=Matrix, shape=self.shape)

    def apply(self, op, right=None, *, left=None):
        """``C << A.apply(binary.times, right=0.85)`` / ``A.apply(binary.minus, left=8)`` / ``A.apply(indexunary.rowindex)``: the operator
        applied to every entry, with the scalar bound as its second (``right``) or first (``left``) argument, or -- an index-unary
        operator -- ``right`` as its thunk (reference core/matrix.py apply -> C ``GrB_Matrix_apply_BinaryOp1st / _BinaryOp2nd /
        _IndexOp_<T>``)."""
        return apply_expression(self, op, right, left, output_type=Matrix, shape=self.shape)

    def __getitem__(self, keys):
        """``A[I, J]`` -> matrix expression, ``A[i, J]`` / ``A[I, j]`` -> vector expression, ``A[i, j]`` -> scalar expression
        (reference core/matrix.py:3020-3090 -> ``GrB_Matrix_extract`` / ``GrB_Col_extract`` / ``GrB_Matrix_extractElement_<T>``)."""
        return _extract(self, keys)

    def __matmul__(self, other):
        return InfixMatMul(self, other)

    # ---- assign (reference core/matrix.py:3092-3300, core/expr.py:404-560 -> GrB_Matrix_assign & co.) -------------------------------
    # ``Matrix.__setitem__`` / ``__delitem__`` are deliberately absent: ``C()[I, J] = A``, ``C()[I, J] << A`` and ``C[I, J] << A`` assign,
    # ``C.remove_element(i, j)`` deletes.
    @staticmethod
    def _is_scalar_index(key):
        def one(k):
            return isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_))

        return isinstance(key, tuple) and len(key) == 2 and one(key[0]) and one(key[1])

    def _resolve_keys(self, keys):
        if not isinstance(keys, tuple) or len(keys) != 2:
            raise TypeError(f"Invalid index for a Matrix: a pair `C[rows, columns]` is required; got {keys!r}")
        return _AxisIndex(keys[0], self._nrows), _AxisIndex(keys[1], self._ncols)

    def _indexed_assigner(self, key, *, mask=None, accum=None, replace=False, opts=None):
        """``C(mask, accum, replace)[I, J]``, ``[i, J]``, ``[I, j]`` on the left of ``<<`` / ``=``"""
        rows, cols = self._resolve_keys(key)
        return _MatrixAssigner(self, rows, cols, mask=mask, accum=accum, replace=replace, opts=opts)

    def _element_assigner(self, key, accum=None):
        """``C()[i, j]`` / ``C(accum)[i, j]`` on the left of ``<<`` / ``=``"""
        rows, cols = self._resolve_keys(key)
        return _MatrixAssigner(self, rows, cols, accum=accum)

    def _assign_scalar_all(self, value, mask=None, accum=None, replace=False, *, opts):
        """``C(mask, accum, replace) << scalar``: the scalar form of GrB_Matrix_assign over GrB_ALL x GrB_ALL (reference
        core/base.py:352-372)."""
        rows, cols = self._resolve_keys((slice(None), slice(None)))
        _MatrixAssigner(self, rows, cols, mask=mask, accum=accum, replace=replace, opts=opts) << value

    def _scalar_value(self, value):
        from .base import Scalar

        if isinstance(value, Scalar):
            if value.is_empty:
                raise ValueError("cannot assign an empty Scalar")
            value = value.value
        if not isinstance(value, (bool, int, float, np.generic)):
            raise TypeError(f"Bad type for arg: {type(value).__name__}")
        return _cast_scalar(value, self.dtype.np_type)

    def remove_element(self, i, j):
        """Delete the entry at (i, j), if there is one (``GrB_Matrix_removeElement``; the reference spells it ``del C[i, j]``).  Costs a
        pass over the matrix: O(nvals)."""
        rows, cols = self._resolve_keys((i, j))
        if rows.scalar is None or cols.scalar is None:
            raise TypeError("remove_element takes one row index and one column index")
        call("GrB_Matrix_removeElement", [self, ctypes.c_uint64(rows.scalar), ctypes.c_uint64(cols.scalar)])


class TransposedMatrix:
    """``A.T``: a view that only flips the descriptor's T0/T1 (reference core/matrix.py:3900-3960)."""

    _is_transposed = True
    ndim = 2
    ss = _SSAccessor()  # A.T.ss.sort(...), A.T.ss.compactify(...): the order flips

    def __init__(self, matrix):
        self._matrix = matrix
        self._nrows, self._ncols = matrix._ncols, matrix._nrows

    dtype = property(lambda self: self._matrix.dtype)
    nrows = property(lambda self: self._nrows)
    ncols = property(lambda self: self._ncols)
    shape = property(lambda self: (self._nrows, self._ncols))
    name = property(lambda self: f"{self._matrix.name}.T")

    @property
    def T(self):
        return self._matrix

    def mxv(self, other, op=_semiring.plus_times):
        return _mxv(self, other, op)

    def mxm(self, other, op=_semiring.plus_times):
        return _mxm(self, other, op)

    def ewise_add(self, other, op=_monoid.plus):
        """``C << A.ewise_add(B, op)``: union of the patterns; ``op`` where both have an entry (reference core/matrix.py
        ewise_add -> C ``GrB_Matrix_eWiseAdd_<opclass>``)."""
        return _ewise(self, other, op, "ewise_add", "GrB_Matrix_eWiseAdd")

    def ewise_mult(self, other, op=_binary.times):
        """``C << A.ewise_mult(B, op)``: intersection of the patterns (reference core/matrix.py ewise_mult -> C
        ``GrB_Matrix_eWiseMult_<opclass>``)."""
        return _ewise(self, other, op, "ewise_mult", "GrB_Matrix_eWiseMult")

    def ewise_union(self, other, op, left_default, right_default):
        """``C << A.T.ewise_union(B, op, left_default, right_default)``: the union runs on the transpose (descriptor T0)."""
        return _ewise_union(self, other, op, left_default, right_default)

    def diag(self, k=0, dtype=None, *, name=None):
        """The k-th diagonal of the transpose: diagonal ``-k`` of the matrix itself."""
        return _diag_vector(self, k, dtype, name)

    def kronecker(self, other, op=_binary.times):
        """``C << A.T.kronecker(B, op)``: the product runs on the transpose (descriptor T0)."""
        return _kronecker(self, other, op)

    def reduce_rowwise(self, op="plus"):
        return _reduce_vector(self, op, "reduce_rowwise", False)

    def reduce_columnwise(self, op="plus"):
        return _reduce_vector(self, op, "reduce_columnwise", True)

    def reduce_scalar(self, op="plus", *, allow_empty=True):
        return _reduce_scalar(self, op, allow_empty)

    def power(self, n, op=_semiring.plus_times):
        return _matrix_power(self, n, op)

    def select(self, op, thunk=None):
        """``A.T.select(op, thunk)``: the selection runs on the transpose (descriptor T0)."""
        return select_expression(self, op, thunk, output_type=Matrix, shape=self.shape, at=True)

    def apply(self, op, right=None, *, left=None):
        """``A.T.apply(op, right)``: the operator runs on the transpose (descriptor T0)."""
        return apply_expression(self, op, right, left, output_type=Matrix, shape=self.shape, at=True)

    def __getitem__(self, keys):
        """``A.T[I, J]``: the same expressions with the roles of rows and columns swapped (descriptor T0)."""
        return _extract(self, keys)

    def __matmul__(self, other):
        return InfixMatMul(self, other)

    def new(self, dtype=None, *, name=None):
        C = Matrix(dtype or self.dtype, self._nrows, self._ncols, name=name)
        call("GrB_transpose", [C, None, None, self._matrix, None])
        return C


class _AxisIndex:
    """One index of ``A[., .]`` resolved against its dimension (reference core/expr.py:176-251, IndexerResolver.parse_index): an int is
    a scalar index; a full ``:`` is ``GrB_ALL``; any other slice is ``np.arange``; a list or a 1-D integer array is taken as it is
    (negative entries count from the end).  Anything else is a ``TypeError``; indices beyond the dimension are the library's
    ``GrB_INDEX_OUT_OF_BOUNDS``."""

    def __init__(self, key, size):
        self.scalar = self.array = None
        self.size = size  # how many indices the axis selects (scalar: None)
        if isinstance(key, (int, np.integer)) and not isinstance(key, (bool, np.bool_)):
            i = int(key)
            if i >= size or i < -size:
                raise IndexError(f"Index out of range: index={i}, size={size}")
            self.scalar, self.size = i + size if i < 0 else i, None
        elif isinstance(key, slice):
            if key != slice(None):
                self.array = np.arange(*key.indices(size), dtype=np.uint64)
                self.size = int(self.array.size)
        elif isinstance(key, np.ndarray) or type(key) is list:
            a = key if isinstance(key, np.ndarray) else (np.asarray(key) if len(key) else np.zeros(0, np.uint64))
            if a.ndim != 1:
                raise TypeError(f"Invalid number of dimensions for index: {a.ndim}")
            if a.dtype.kind not in "iu":
                raise TypeError(f"Invalid dtype for index: {a.dtype}")
            if a.dtype.kind == "i" and a.size and a.min() < 0:
                a = np.where(a < 0, a + size, a)
                if a.min() < 0:
                    raise IndexError(f"Index out of range: index={int(a.min()) - size}, size={size}")
            self.array = np.ascontiguousarray(a, dtype=np.uint64)
            self.size = int(self.array.size)
        elif isinstance(key, (Mask, BaseType, TransposedMatrix)):
            raise TypeError(f"Invalid type for index: {type(key).__name__}.\nIf you want to apply a mask, perhaps do something like `x.dup(mask=M.S)`.")
        else:
            raise TypeError(f"Invalid type for index: {type(key).__name__}; integers, slices, lists and 1-D integer arrays are supported")

    @property
    def cargs(self):
        """(pointer, count) as the C entry points take an index list"""
        if self.array is None:
            return _lib.all_indices(), ctypes.c_uint64(self.size)
        return _iptr(self.array), ctypes.c_uint64(self.size)


class _MatrixElementExpr(ScalarExpression):
    """``A[i, j]``: read with ``.new()`` / ``.value`` / a comparison (reference core/matrix.py:3020-3050)."""

    def __init__(self, matrix, row, col, at=False):
        self.parent, self.row, self.col, self._at = matrix, row, col, at
        super().__init__(self._read, matrix.dtype)

    def _read(self):
        A = self.parent
        out = np.ctypeslib.as_ctypes_type(A.dtype.np_type)()
        info = getattr(_lib.lib, f"GrB_Matrix_extractElement_{A.dtype.name}")(ctypes.byref(out), A._handle, self.row, self.col)
        if info == _lib.GrB_NO_VALUE:
            return None
        from .exceptions import check_status

        check_status(info, A)
        return A.dtype.np_type.type(out.value).item()

    def _assigner(self, up=None):
        one = lambda i, dim: _AxisIndex(i, dim)  # noqa: E731
        A = self.parent
        if self._at:
            raise TypeError("'TransposedMatrix' object does not support item assignment")
        rows, cols = one(self.row, A._nrows), one(self.col, A._ncols)
        if up is None:
            return _MatrixAssigner(A, rows, cols)
        return _MatrixAssigner(A, rows, cols, mask=up.mask, accum=up.accum, replace=up.replace, opts=up.opts, sub=True)

    def __call__(self, *args, **kwargs):
        """``C[i, j](accum=op) << x`` (reference core/matrix.py:3092-3140)"""
        return self._assigner(self.parent(*args, **kwargs))

    def __lshift__(self, value):
        self._assigner() << value

    update = __lshift__


def _extract(A, keys):
    if not isinstance(keys, tuple) or len(keys) != 2:
        raise TypeError(f"Invalid index for a Matrix: a pair `A[rows, columns]` is required; got {keys!r}")
    base, at = A._matrix, A._is_transposed
    rows, cols = _AxisIndex(keys[0], A._nrows), _AxisIndex(keys[1], A._ncols)
    if rows.scalar is not None and cols.scalar is not None:
        i, j = (cols.scalar, rows.scalar) if at else (rows.scalar, cols.scalar)
        return _MatrixElementExpr(base, i, j, at)
    if rows.scalar is None and cols.scalar is None:
        expr = _IndexedMatrix("extract", "GrB_Matrix_extract", [base, *rows.cargs, *cols.cargs], op=None, output_type=Matrix,
                              shape=(rows.size, cols.size), at=at, dtype=base.dtype)
    else:
        # A[i, J] is the reference's spelling of GrB_Col_extract with T0 (row i of A); on A.T the roles swap
        row_form = rows.scalar is not None
        lst, j = (cols, rows.scalar) if row_form else (rows, cols.scalar)
        expr = _IndexedMatrix("extract", "GrB_Col_extract", [base, *lst.cargs, ctypes.c_uint64(j)], op=None, output_type=Vector,
                              shape=(lst.size,), at=row_form != at, dtype=base.dtype)
    expr._index_arrays = (rows.array, cols.array)  # (the C call reads them: kept alive with the expression)
    expr._target = (A, rows, cols)
    return expr


class _IndexedMatrix(Expression):
    """``A[I, J]`` / ``A[i, J]`` / ``A[I, j]``: on the right of ``<<`` (or with ``.new()``) it extracts; on the left it is an assign
    target -- ``C[I, J] << A``, ``C[I, J]() << A``, ``C[i, J](accum=op) << v`` (the reference's AmbiguousAssignOrExtract, core/expr.py:
    240-400; the matrix counterpart of ``IndexedVector``)."""

    def _assigner(self, up=None):
        A, rows, cols = self._target
        if A._is_transposed:
            raise TypeError("'TransposedMatrix' object does not support item assignment")
        if up is None:
            return _MatrixAssigner(A, rows, cols)
        return _MatrixAssigner(A, rows, cols, mask=up.mask, accum=up.accum, replace=up.replace, opts=up.opts, sub=True)

    def __call__(self, *args, **kwargs):
        if self._target[0]._is_transposed:
            raise TypeError("'TransposedMatrix' object does not support item assignment")
        return self._assigner(self._target[0](*args, **kwargs))

    def __lshift__(self, value):
        self._assigner() << value

    update = __lshift__


class _MatrixAssigner:
    """The left side of a Matrix assign with its output parameters resolved: ``<<`` / ``update`` run it.
      both indices lists / slices   GrB_Matrix_assign (a Matrix or ``A.T``), GrB_Matrix_assign_<T> / _Scalar (a number or a Scalar)
      one index an integer          GrB_Row_assign / GrB_Col_assign (a Vector; a number under a Vector mask), else the scalar form
      both integers                 GrB_Matrix_setElement_<T>; an empty Scalar removes the element
    ``sub``: the parameters came behind the index (``C[I, J](mask) << A``), the reference's SUBassign, whose mask has the shape of the
    region: only the spellings where that is the same thing as assign are accepted."""

    def __init__(self, parent, rows, cols, *, mask=None, accum=None, replace=False, opts=None, sub=False):
        self.parent, self.rows, self.cols = parent, rows, cols
        self.mask, self.accum, self.replace, self.opts, self.sub = mask, accum, replace, opts or {}, sub

    def _desc(self, mask, **extra):
        from .descriptor import lookup as descriptor_lookup

        complement, structure = (mask.complement, mask.structure) if mask is not None else (False, False)
        return descriptor_lookup(mask_complement=complement, mask_structure=structure, output_replace=self.replace, **extra, **self.opts)

    def __lshift__(self, value):
        from .base import Scalar, _is_python_scalar

        C, rows, cols, mask, accum = self.parent, self.rows, self.cols, self.mask, self.accum
        where = f"Matrix[{'i' if rows.scalar is not None else 'I'}, {'j' if cols.scalar is not None else 'J'}] = ..."
        if isinstance(value, InfixMatMul):
            value = value.new()
        if isinstance(value, Expression):
            value = value.new()
        n_scalar = (rows.scalar is not None) + (cols.scalar is not None)
        if isinstance(value, (list, np.ndarray)):
            if n_scalar == 2:
                raise TypeError(f"Bad type for arg `value` in {where}: {type(value).__name__}")
            value = _dense_value(np.asarray(value), rows, cols, C)
        is_scalar = isinstance(value, Scalar) or _is_python_scalar(value)
        vmask = mask is not None and isinstance(mask.parent, Vector)
        if accum is not None:
            accum = get_typed_op(accum, C.dtype, kind="binary")
            if accum.opclass == "Monoid":
                accum = accum.binaryop
        if n_scalar == 2:
            if mask is not None:
                raise TypeError("Unable to use Vector mask on single element assignment to a Matrix" if vmask else
                                "Single element assign does not accept a submask")
            if not is_scalar:
                raise TypeError(f"Bad type for arg `value` in {where}: {type(value).__name__}")
            return self._set_element(value, accum)
        if n_scalar == 1:
            row_form = rows.scalar is not None
            lst, idx = (cols, rows.scalar) if row_form else (rows, cols.scalar)
            if is_scalar and vmask:
                # (a number into a row / column under a Vector mask: the vector form needs a vector -- a full one of the list's length)
                value = Vector.from_coo(np.arange(lst.size, dtype=np.uint64), np.full(lst.size, C._scalar_value(value)), dtype=C.dtype,
                                        size=lst.size)
                is_scalar = False
            if isinstance(value, Vector):
                if mask is not None and not vmask:
                    raise TypeError("Unable to use Matrix mask on a row or column assignment of a Vector; use a Vector mask")
                i = ctypes.c_uint64(idx)
                if row_form:
                    return call("GrB_Row_assign", [C, mask, accum, value, i, *lst.cargs, self._desc(mask)])
                return call("GrB_Col_assign", [C, mask, accum, value, *lst.cargs, i, self._desc(mask)])
            if not is_scalar:
                raise TypeError(f"Bad type for arg `value` in {where}: {type(value).__name__}")
            one = _AxisIndex([idx], C._nrows if row_form else C._ncols)
            rows, cols = (one, cols) if row_form else (rows, one)
        if vmask:
            raise TypeError("Unable to use Vector mask on Matrix assignment to a Matrix")
        if self.sub and mask is not None and not (rows.array is None and cols.array is None and n_scalar == 0):
            raise TypeError("C[I, J](mask) << value is a SUBassign (the mask has the shape of the region), which this library does not have; "
                            "write C(mask)[I, J] << value with a mask of the shape of C")
        if isinstance(value, (Matrix, TransposedMatrix)) and n_scalar == 0:
            desc = self._desc(mask, transpose_first=value._is_transposed)
            return call("GrB_Matrix_assign", [C, mask, accum, value._matrix, *rows.cargs, *cols.cargs, desc])
        if not is_scalar:
            raise TypeError(f"Bad type for arg `value` in {where}: {type(value).__name__}")
        if isinstance(value, Scalar):
            from .base import GrBScalarArg

            return call("GrB_Matrix_assign_Scalar", [C, mask, accum, GrBScalarArg(value), *rows.cargs, *cols.cargs, self._desc(mask)])
        ctype = np.ctypeslib.as_ctypes_type(C.dtype.np_type)
        return call(f"GrB_Matrix_assign_{C.dtype.name}", [C, mask, accum, ctype(C._scalar_value(value).item()), *rows.cargs, *cols.cargs,
                                                          self._desc(mask)])

    update = __lshift__

    def _set_element(self, value, accum):
        from .base import Scalar, _apply_host_binary

        C, i, j = self.parent, self.rows.scalar, self.cols.scalar
        if isinstance(value, Scalar) and value.is_empty:
            return C.remove_element(i, j)
        x = C._scalar_value(value)
        if accum is not None:
            old = _MatrixElementExpr(C, i, j).value
            if old is not None:
                x = C.dtype.np_type.type(_apply_host_binary(accum.name, C.dtype.np_type.type(old), x))
        ctype = np.ctypeslib.as_ctypes_type(C.dtype.np_type)
        call(f"GrB_Matrix_setElement_{C.dtype.name}", [C, ctype(x.item()), ctypes.c_uint64(i), ctypes.c_uint64(j)])


def _dense_value(a, rows, cols, C):
    """A list / array on the right of an assign: a full Matrix or Vector of the region's shape (reference tests/test_matrix.py:1759-1781)."""
    want = tuple(ax.size for ax in (rows, cols) if ax.scalar is None)
    if a.shape != want:
        raise ValueError(f"shape mismatch: value array of shape {a.shape} does not match indexing of shape {want}")
    if a.ndim == 1:
        return Vector.from_coo(np.arange(a.size, dtype=np.uint64), a, size=a.size)
    r, c = np.divmod(np.arange(a.size, dtype=np.uint64), np.uint64(max(a.shape[1], 1)))
    return Matrix.from_coo(r, c, a.ravel(), nrows=a.shape[0], ncols=a.shape[1])


def _reduce_vector(A, op, method_name, transpose):
    """``w << A.reduce_rowwise(monoid)`` / ``reduce_columnwise`` (reference core/matrix.py:2636-2710 -> ``GrB_Matrix_reduce_Monoid``;
    column-wise = row-wise over the transpose, descriptor T0).  An aggregator is either its monoid or, for ``count`` /
    ``exists``, the mat-vec ``semiring(A @ init)`` with a dense iso vector (reference core/operator/agg.py:264-283)."""
    from .operators import Aggregator
    from .operators import monoid as _monoid_ns

    at = A._is_transposed != transpose
    base = A._matrix
    if isinstance(op, Aggregator):
        if op.semiring is not None:
            view = base.T if at else base
            init = Vector(op.any_dtype, view._ncols, name="init")
            init[:] = 1
            expr = _mxv(view, init, op.semiring[op.any_dtype])
            expr.method_name = method_name
            return expr
        op = op.monoid
    op = get_typed_op(op, A.dtype, kind="binary")
    if op.opclass == "BinaryOp":
        if not hasattr(_monoid_ns, op.name):
            raise TypeError(f"Expected type: Monoid; got BinaryOp `{op!r}`")
        op = getattr(_monoid_ns, op.name)[A.dtype]
    out_size = base._ncols if at else base._nrows
    return Expression(method_name, "GrB_Matrix_reduce_Monoid", [base], op=op, output_type=Vector, shape=(out_size,), at=at)


def _reduce_scalar(A, op, allow_empty):
    from .base import ScalarExpression
    from .operators import Aggregator

    base = A._matrix
    if isinstance(op, Aggregator) and op.semiring is not None:
        count = op.name == "count"

        def compute_agg():
            nv = base.nvals
            if nv == 0 and (allow_empty or not count):
                return None if allow_empty else 0
            return int(nv) if count else 1

        return ScalarExpression(compute_agg, op.any_dtype)
    mon = op.monoid if isinstance(op, Aggregator) else op
    rows = _reduce_vector(base, mon, "reduce_scalar", False)

    def compute():
        return rows.new().reduce(mon, allow_empty=allow_empty).value

    return ScalarExpression(compute, rows.dtype)


def _power(updater, A, n, op):
    """Repeated squaring over the mxm path (reference core/matrix.py:99-155): A^2, A^4, ... are formed in ``square`` and
    multiplied into ``result`` for each set bit of ``n``; the last product goes through the caller's updater so that its
    mask / accum / replace apply to the final multiplication only."""
    opts = updater.opts
    if n == 0:
        ident = op.parent.binaryop.monoid.identity(A.dtype)
        idx = np.arange(A._nrows, dtype=np.uint64)
        D = Matrix.from_coo(idx, idx, np.full(A._nrows, ident), dtype=A.dtype, nrows=A._nrows, ncols=A._ncols, name="M_diag")
        updater << PowerCopy(D)
        return
    if n == 1:
        updater << PowerCopy(A)
        return
    result = square = None  # square = A^(2^k) once k >= 1; result = product of the squares of the bits seen so far
    owned = False           # result is a matrix of ours (not A itself)
    k = 0
    while True:
        n, bit = divmod(n, 2)
        if k:
            src = A if square is None else square
            squaring = _mxm(src, src, op)
            if n == 0 and result is None:  # n was a power of two: the last squaring is the answer
                updater << squaring
                return
            if square is None:
                square = squaring.new(name="Squares", **opts)
            else:
                square(**opts) << squaring
        k += 1
        if not bit:
            continue
        cur = A if square is None else square
        if result is None:
            result, owned = (A, False) if square is None else (square.dup(name="Power"), True)
        elif n == 0:
            updater << _mxm(result, cur, op)
            return
        elif not owned:
            result, owned = _mxm(result, cur, op).new(name="Power", **opts), True
        else:
            result(**opts) << _mxm(result, cur, op)


class PowerCopy:
    """``C << A`` for the degenerate powers (n = 0, 1): a copy through ``GrB_transpose`` with descriptor T0."""

    def __init__(self, matrix):
        self.matrix = matrix


class PowerExpression:
    """``A.power(n, op)`` (reference core/matrix.py:2840-2905): evaluated by ``_power`` when assigned."""

    def __init__(self, A, n, op):
        self.A, self.n, self.op = A, n, op
        self.shape = (A._nrows, A._ncols)
        self.dtype = op.return_type

    def new(self, dtype=None, *, mask=None, name=None, **opts):
        out = Matrix(dtype or self.dtype, *self.shape, name=name)
        if mask is None:
            out(**opts) << self
        else:
            out(mask=mask, **opts) << self
        return out


def _matrix_power(A, n, op):
    from numbers import Integral

    if A._nrows != A._ncols:
        raise DimensionMismatch(f"power only works for square Matrix; shape is {A.shape}")
    if isinstance(n, bool) or not (isinstance(n, (Integral, np.integer)) or (isinstance(n, float) and n.is_integer())):
        raise TypeError(f"n must be a nonnegative integer; got bad type: {type(n)}")
    N = int(n)
    if N < 0:
        raise ValueError(f"n must be a nonnegative integer; got: {N}")
    op = get_typed_op(op, A.dtype, kind="semiring")
    if N == 0 and op.parent.binaryop.monoid is None:
        raise ValueError(
            f"Binary operator of {op} semiring does not have a monoid with an identity. "
            "When n=0, the result is a diagonal matrix with values equal to the "
            "identity of the binaryop, so the binaryop must be associated with a monoid."
        )
    return PowerExpression(A, N, op)


def _mxv(A, v, op):
    if not isinstance(v, Vector):
        raise TypeError(f"Expected type: Vector; got {type(v).__name__}")
    op = get_typed_op(op, A.dtype, v.dtype, kind="semiring")
    expr = Expression("mxv", "GrB_mxv", [A._matrix, v], op=op, output_type=Vector, shape=(A._nrows,),
                      at=A._is_transposed)
    if A._ncols != v._size:
        expr._force_library_error()
    return expr


def _ewise(A, B, op, method_name, cfunc):
    if not isinstance(B, (Matrix, TransposedMatrix)):
        raise TypeError(f"Expected type: Matrix; got {type(B).__name__}")
    op = get_typed_op(op, A.dtype, B.dtype, kind="binary")
    expr = Expression(method_name, f"{cfunc}_{op.opclass}", [A._matrix, B._matrix], op=op, output_type=Matrix, shape=A.shape,
                      at=A._is_transposed, bt=B._is_transposed)
    if A.shape != B.shape:
        expr._force_library_error()
    return expr


def _ewise_union(A, B, op, left_default, right_default):
    from .base import union_expression

    if not isinstance(B, (Matrix, TransposedMatrix)):
        raise TypeError(f"Expected type: Matrix; got {type(B).__name__}")
    expr = union_expression(A, B, op, left_default, right_default, kind="Matrix", output_type=Matrix, shape=A.shape,
                            at=A._is_transposed, bt=B._is_transposed)
    if A.shape != B.shape:
        expr._force_library_error()
    return expr


def diag_offset(k):
    """The diagonal number of ``diag(k)``: an int, or a Scalar that holds one (reference tests/test_vector.py:1459-1490)."""
    from .base import Scalar

    if isinstance(k, Scalar):
        if k.is_empty:
            raise ValueError("diag: k is an empty Scalar")
        k = k.value
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise TypeError(f"diag: k must be an integer or a Scalar that holds one; got {type(k).__name__}")
    return int(k)


def _diag_vector(A, k, dtype, name):
    base = A._matrix
    k = -diag_offset(k) if A._is_transposed else diag_offset(k)
    m, n = base._nrows, base._ncols
    size = min(m, n - k) if 0 <= k < n else (min(m + k, n) if -m < k < 0 else 0)
    v = Vector(base.dtype if dtype is None else dtype, size, name=name)
    call("GxB_Vector_diag", [v, base, ctypes.c_int64(k), None])
    return v


def _kronecker(A, B, op):
    if not isinstance(B, (Matrix, TransposedMatrix)):
        raise TypeError(f"Expected type: Matrix; got {type(B).__name__}")
    op = get_typed_op(op, A.dtype, B.dtype, kind="binary")  # (a BinaryOp or a Monoid; a Semiring is a TypeError, as in the reference)
    return Expression("kronecker", f"GrB_Matrix_kronecker_{op.opclass}", [A._matrix, B._matrix], op=op, output_type=Matrix,
                      shape=(A._nrows * B._nrows, A._ncols * B._ncols), at=A._is_transposed, bt=B._is_transposed)


def _mxm(A, B, op):
    if not isinstance(B, (Matrix, TransposedMatrix)):
        raise TypeError(f"Expected type: Matrix; got {type(B).__name__}")
    op = get_typed_op(op, A.dtype, B.dtype, kind="semiring")
    expr = Expression("mxm", "GrB_mxm", [A._matrix, B._matrix], op=op, output_type=Matrix,
                      shape=(A._nrows, B._ncols), at=A._is_transposed, bt=B._is_transposed)
    if A._ncols != B._nrows:
        expr._force_library_error()
    return expr
