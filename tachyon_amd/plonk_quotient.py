"""The Halo2 quotient h(X) on the GPU over the C-ABI ("PLONK quotient").

Reference: tachyon/zk/plonk/vanishing/ -- graph_evaluator.h (the flattening of
an expression, with its folding rules), calculation.h, value_source.h,
custom_gate_evaluator.h, circuit_polynomial_builder.h:199-245 (the Scroll
shape), vanishing_utils.h (zeta, the interleave, the division and the coset
IFFT) -- and the closed forms of permutation_evaluator.h:25-108,
lookup/halo2/evaluator.h and shuffle/evaluator.h.

`GraphEvaluator` flattens small expression-tuple trees:
    ("const", v)  ("fixed" | "advice" | "instance", column, rotation)
    ("challenge", index)  ("neg", e)  ("sum", a, b)  ("product", a, b)
    ("scaled", e, v)
with v a canonical int.  Polynomials and columns are Montgomery bytes / numpy
(host) or CUDA tensors, as in `tachyon_amd.plonk`.
"""
import ctypes

from . import params as P
from ._lib import lib
from .msm import _ptr
from .plonk import FIELDS, _Columns, _is_cuda, _mont

# value_source.h's kinds and calculation.h's ops, in their order
CONSTANT, INTERMEDIATE, FIXED, ADVICE, INSTANCE, CHALLENGE, BETA, GAMMA, THETA, Y, PREVIOUS_VALUE = range(11)
ADD, SUB, MUL, SQUARE, DOUBLE, NEGATE, HORNER, STORE = range(8)
GATES, PERMUTATION, LOOKUP, SHUFFLE = range(4)
COLUMN_KINDS = {"fixed": FIXED, "advice": ADVICE, "instance": INSTANCE}
PHASES = ("transforms", "gates", "permutation", "lookups", "shuffles", "scatter", "ifft")


class QSource(ctypes.Structure):
    """tachyon_mi355x_quotient_source"""
    _fields_ = [("kind", ctypes.c_uint32), ("index", ctypes.c_uint32), ("rotation_index", ctypes.c_uint32)]


class QCalc(ctypes.Structure):
    """tachyon_mi355x_quotient_calc"""
    _fields_ = [("op", ctypes.c_uint32), ("a", QSource), ("b", QSource), ("parts_begin", ctypes.c_uint32),
                ("parts_count", ctypes.c_uint32), ("target", ctypes.c_uint32)]


class QGraph(ctypes.Structure):
    """tachyon_mi355x_quotient_graph"""
    _fields_ = [("calcs", ctypes.POINTER(QCalc)), ("num_calcs", ctypes.c_size_t),
                ("parts", ctypes.POINTER(QSource)), ("num_parts", ctypes.c_size_t),
                ("constants", ctypes.c_void_p), ("num_constants", ctypes.c_size_t),
                ("rotations", ctypes.POINTER(ctypes.c_int32)), ("num_rotations", ctypes.c_size_t),
                ("num_intermediates", ctypes.c_size_t)]


_VPP = ctypes.POINTER(ctypes.c_void_p)


class QTable(ctypes.Structure):
    """tachyon_mi355x_quotient_table"""
    _fields_ = [("fixed", _VPP), ("num_fixed", ctypes.c_size_t), ("advice", _VPP), ("num_advice", ctypes.c_size_t),
                ("instance", _VPP), ("num_instance", ctypes.c_size_t), ("challenges", ctypes.c_void_p),
                ("num_challenges", ctypes.c_size_t)]


class QParams(ctypes.Structure):
    """tachyon_mi355x_quotient_params"""
    _fields_ = [("field", ctypes.c_int), ("n", ctypes.c_size_t), ("cs_degree", ctypes.c_uint32),
                ("last_row", ctypes.c_int32), ("theta", ctypes.c_void_p), ("beta", ctypes.c_void_p),
                ("gamma", ctypes.c_void_p), ("y", ctypes.c_void_p), ("l_first", ctypes.c_void_p),
                ("l_last", ctypes.c_void_p), ("l_active_row", ctypes.c_void_p)]


class QGroup(ctypes.Structure):
    """tachyon_mi355x_quotient_group"""
    _fields_ = [("kind", ctypes.c_uint32), ("graph", ctypes.POINTER(QGraph)), ("graph2", ctypes.POINTER(QGraph)),
                ("z", _VPP), ("num_z", ctypes.c_size_t), ("a_perm", ctypes.c_void_p), ("s_perm", ctypes.c_void_p),
                ("perm_columns", ctypes.POINTER(QSource)), ("num_perm_columns", ctypes.c_size_t), ("sigmas", _VPP),
                ("x_scale", ctypes.c_void_p), ("omega", ctypes.c_void_p), ("delta", ctypes.c_void_p)]


class QSystem(ctypes.Structure):
    """tachyon_mi355x_quotient_system"""
    _fields_ = [("gates", ctypes.POINTER(QGraph)), ("perm_columns", ctypes.POINTER(QSource)),
                ("num_perm_columns", ctypes.c_size_t), ("sigmas", _VPP), ("lookups", ctypes.POINTER(QGraph)),
                ("num_lookups", ctypes.c_size_t), ("shuffles", ctypes.POINTER(QGraph)),
                ("num_shuffles", ctypes.c_size_t)]


class QCircuit(ctypes.Structure):
    """tachyon_mi355x_quotient_circuit"""
    _fields_ = [("table", QTable), ("perm_z", _VPP), ("num_perm_z", ctypes.c_size_t), ("lookup_z", _VPP),
                ("lookup_a_perm", _VPP), ("lookup_s_perm", _VPP), ("shuffle_z", _VPP)]


def tile_rows() -> int:
    """Rows one workgroup of the evaluator owns."""
    return lib().tachyon_mi355x_quotient_tile_rows()


def fast_slots() -> int:
    """Intermediates of a lowered program that live in LDS; more spill."""
    return lib().tachyon_mi355x_quotient_fast_slots()


def held_bytes() -> int:
    """Device memory the last quotient_h_poly call held when it returned."""
    return lib().tachyon_mi355x_quotient_held_bytes()


def last_timings() -> dict:
    """Milliseconds (stream events) of the last call's phases."""
    ms = (ctypes.c_float * len(PHASES))()
    lib().tachyon_mi355x_quotient_last_timings(ms)
    return dict(zip(PHASES, [float(x) for x in ms]))


def extended_k(n: int, cs_degree: int) -> int:
    """The least e with 2^e >= n (cs_degree - 1): the extended domain's log size."""
    e = n.bit_length() - 1
    while (1 << e) < n * (cs_degree - 1):
        e += 1
    return e


def get_zeta(field: str = "bn254_fr", vendor: str = "scroll") -> bytes:
    """GetHalo2Zeta (vanishing_utils.h:25-63) as Montgomery bytes: the cube
    root of unity g^((r - 1) / 3), squared for PSE.  The reference defines it
    for BN254 only; other fields take the same formula with their generator."""
    r, _, g = P.FIELDS[field]
    if (r - 1) % 3 or vendor not in ("scroll", "pse"):
        raise ValueError("zeta: r - 1 divisible by 3, vendor scroll or pse")
    z = pow(g, (r - 1) // 3, r)
    return _mont(field, z * z % r if vendor == "pse" else z)


class GraphEvaluator:
    """graph_evaluator.h over expression tuples.  A source is a tuple (kind,
    index, rotation_index); a calculation (op, a, b, parts) with parts a tuple
    of sources (Horner only), its target its position."""

    def __init__(self, field: str = "bn254_fr"):
        self.field = field
        self.p = P.FIELDS[field][0]
        self.constants = [0, 1, 2]
        self.rotations = []
        self.calculations = []

    @property
    def num_intermediates(self):
        return len(self.calculations)

    # -- the building blocks ---------------------------------------------------
    def add_constant(self, v):
        v %= self.p
        if v not in self.constants:
            self.constants.append(v)
        return (CONSTANT, self.constants.index(v), 0)

    def add_rotation(self, r):
        if r not in self.rotations:
            self.rotations.append(r)
        return self.rotations.index(r)

    def add_calculation(self, op, a, b=None, parts=()):
        calc = (op, a, b, tuple(parts))
        if calc not in self.calculations:
            self.calculations.append(calc)
        return (INTERMEDIATE, self.calculations.index(calc), 0)

    @staticmethod
    def _le(a, b):
        """ValueSource::operator<= (value_source.h): by kind, then index, then rotation index."""
        if a[0] != b[0]:
            return a[0] < b[0]
        if a[0] in (FIXED, ADVICE, INSTANCE):
            return a[2] <= b[2] if a[1] == b[1] else a[1] < b[1]
        if a[0] in (CONSTANT, INTERMEDIATE, CHALLENGE):
            return a[1] <= b[1]
        return True

    def add_expression(self, e):
        """GraphEvaluator::Evaluate with its folding rules."""
        zero, one, two = (CONSTANT, 0, 0), (CONSTANT, 1, 0), (CONSTANT, 2, 0)
        tag = e[0]
        if tag == "const":
            return self.add_constant(e[1])
        if tag in COLUMN_KINDS:
            return self.add_calculation(STORE, (COLUMN_KINDS[tag], e[1], self.add_rotation(e[2])))
        if tag == "challenge":
            return self.add_calculation(STORE, (CHALLENGE, e[1], 0))
        if tag == "neg":
            if e[1][0] == "const":
                return self.add_constant(-e[1][1])
            r = self.add_expression(e[1])
            return r if r == zero else self.add_calculation(NEGATE, r)
        if tag == "sum":
            left = self.add_expression(e[1])
            if e[2][0] == "neg":
                right = self.add_expression(e[2][1])
                if left == zero:
                    return self.add_calculation(NEGATE, right)
                return left if right == zero else self.add_calculation(SUB, left, right)
            right = self.add_expression(e[2])
            if left == zero:
                return right
            if right == zero:
                return left
            return self.add_calculation(ADD, left, right) if self._le(left, right) \
                else self.add_calculation(ADD, right, left)
        if tag == "product":
            left, right = self.add_expression(e[1]), self.add_expression(e[2])
            if left == zero or right == zero:
                return zero
            if left == one:
                return right
            if right == one:
                return left
            if left == two:
                return self.add_calculation(DOUBLE, right)
            if right == two:
                return self.add_calculation(DOUBLE, left)
            if left == right:
                return self.add_calculation(SQUARE, left)
            return self.add_calculation(MUL, left, right) if self._le(left, right) \
                else self.add_calculation(MUL, right, left)
        if tag == "scaled":
            s = e[2] % self.p
            if s == 0:
                return zero
            if s == 1:
                return self.add_expression(e[1])
            c = self.add_constant(s)
            return self.add_calculation(MUL, self.add_expression(e[1]), c)
        raise ValueError(f"unknown expression {tag!r}")

    # -- the three Construct shapes ---------------------------------------------
    def _compress(self, expressions):
        parts = [self.add_expression(x) for x in expressions]
        return self.add_calculation(HORNER, (CONSTANT, 0, 0), (THETA, 0, 0), parts)

    @classmethod
    def for_gates(cls, polys, field="bn254_fr"):
        """CustomGateEvaluator::Construct: every gate polynomial, then
        Horner(PreviousValue, parts, Y)."""
        g = cls(field)
        parts = [g.add_expression(x) for x in polys]
        g.add_calculation(HORNER, (PREVIOUS_VALUE, 0, 0), (Y, 0, 0), parts)
        return g

    @classmethod
    def for_lookup(cls, inputs, tables, field="bn254_fr"):
        """lookup::halo2::Evaluator::Construct: (A_compressed + beta)(S_compressed + gamma)."""
        g = cls(field)
        a, s = g._compress(inputs), g._compress(tables)
        left = g.add_calculation(ADD, a, (BETA, 0, 0))
        right = g.add_calculation(ADD, s, (GAMMA, 0, 0))
        g.add_calculation(MUL, left, right)
        return g

    @classmethod
    def for_shuffle(cls, inputs, shuffles, field="bn254_fr"):
        """shuffle::Evaluator::Construct: the pair A_compressed + gamma, S_compressed + gamma."""
        pair = []
        for exprs in (inputs, shuffles):
            g = cls(field)
            g.add_calculation(ADD, g._compress(exprs), (GAMMA, 0, 0))
            pair.append(g)
        return tuple(pair)

    # -- the C-ABI's view ---------------------------------------------------------
    def fill(self, dst: QGraph, keep):
        calcs = (QCalc * max(1, len(self.calculations)))()
        parts = []
        for i, (op, a, b, ps) in enumerate(self.calculations):
            c = calcs[i]
            c.op, c.target = op, i
            c.a = QSource(*a)
            c.b = QSource(*(b if b is not None else (0, 0, 0)))
            c.parts_begin, c.parts_count = len(parts), len(ps)
            parts.extend(ps)
        part_arr = (QSource * max(1, len(parts)))(*[QSource(*s) for s in parts])
        consts = ctypes.create_string_buffer(b"".join(_mont(self.field, v) for v in self.constants))
        rots = (ctypes.c_int32 * max(1, len(self.rotations)))(*self.rotations)
        keep.extend([calcs, part_arr, consts, rots])
        dst.calcs, dst.num_calcs = calcs, len(self.calculations)
        dst.parts, dst.num_parts = part_arr, len(parts)
        dst.constants, dst.num_constants = ctypes.cast(consts, ctypes.c_void_p), len(self.constants)
        dst.rotations, dst.num_rotations = rots, len(self.rotations)
        dst.num_intermediates = len(self.calculations)


class _Args(_Columns):
    """The ctypes images of a call and what keeps them alive."""

    def __init__(self, field, n):
        super().__init__(n, "a column or polynomial is n 32-byte elements")
        self.field = field

    def column(self, x):
        return None if x is None else self.ptr(x)

    def columns(self, xs):
        arr = (ctypes.c_void_p * max(1, len(xs)))(*[self.column(x) for x in xs])
        self.keep.append(arr)
        return ctypes.cast(arr, _VPP)

    def elem(self, b):
        if b is None:
            return None
        if len(bytes(b)) != 32:
            raise ValueError("a field element is 32 Montgomery bytes")
        buf = ctypes.create_string_buffer(bytes(b), 32)
        self.keep.append(buf)
        return ctypes.cast(buf, ctypes.c_void_p)

    def table(self, dst: QTable, fixed, advice, instance, challenges):
        dst.fixed, dst.num_fixed = self.columns(fixed), len(fixed)
        dst.advice, dst.num_advice = self.columns(advice), len(advice)
        dst.instance, dst.num_instance = self.columns(instance), len(instance)
        ch = ctypes.create_string_buffer(b"".join(bytes(c) for c in challenges), max(1, 32 * len(challenges)))
        self.keep.append(ch)
        dst.challenges, dst.num_challenges = ctypes.cast(ch, ctypes.c_void_p), len(challenges)

    def params(self, cs_degree, last_row, theta, beta, gamma, y, l_first, l_last, l_active_row):
        p = QParams()
        p.field, p.n, p.cs_degree, p.last_row = FIELDS[self.field], self.n, cs_degree, last_row
        p.theta, p.beta, p.gamma, p.y = self.elem(theta), self.elem(beta), self.elem(gamma), self.elem(y)
        p.l_first, p.l_last, p.l_active_row = self.column(l_first), self.column(l_last), self.column(l_active_row)
        return p

    def graph(self, g):
        if g is None:
            return None
        q = QGraph()
        g.fill(q, self.keep)
        self.keep.append(q)
        return ctypes.pointer(q)

    def graphs(self, gs):
        arr = (QGraph * max(1, len(gs)))()
        for i, g in enumerate(gs):
            g.fill(arr[i], self.keep)
        self.keep.append(arr)
        return arr

    def sources(self, cols):
        arr = (QSource * max(1, len(cols)))(*[QSource(COLUMN_KINDS[k] if isinstance(k, str) else k, i, 0)
                                             for k, i in cols])
        self.keep.append(arr)
        return arr


def _part_args(field, n, kind, cs_degree, last_row, theta, beta, gamma, y, fixed, advice, instance, challenges, l_first,
               l_last, l_active_row, graph, graph2, z, a_perm, s_perm, perm_columns, sigmas, x_scale, omega, delta):
    a = _Args(field, n)
    p = a.params(cs_degree, last_row, theta, beta, gamma, y, l_first, l_last, l_active_row)
    t = QTable()
    a.table(t, list(fixed), list(advice), list(instance), list(challenges))
    g = QGroup()
    g.kind = kind
    g.graph, g.graph2 = a.graph(graph), a.graph(graph2)
    g.z, g.num_z = a.columns(list(z)), len(z)
    g.a_perm, g.s_perm = a.column(a_perm), a.column(s_perm)
    g.perm_columns, g.num_perm_columns = a.sources(list(perm_columns)), len(perm_columns)
    g.sigmas = a.columns(list(sigmas))
    g.x_scale, g.omega, g.delta = a.elem(x_scale), a.elem(omega), a.elem(delta)
    return a, p, t, g


def quotient_evaluate_part(field, n, kind, acc, *, cs_degree=3, last_row=0, theta, beta, gamma, y, fixed=(), advice=(),
                           instance=(), challenges=(), l_first=None, l_last=None, l_active_row=None, graph=None,
                           graph2=None, z=(), a_perm=None, s_perm=None, perm_columns=(), sigmas=(), x_scale=None,
                           omega=None, delta=None):
    """tachyon_mi355x_quotient_evaluate_part: one term group (GATES,
    PERMUTATION, LOOKUP or SHUFFLE) on caller-held evaluations of one coset.
    acc: the accumulator, n elements -- a CUDA tensor is updated in place and
    returned, bytes / numpy give the new accumulator as bytes.  perm_columns:
    (kind, index) pairs with kind "fixed" / "advice" / "instance".  Returns
    None on a refusal."""
    a, p, t, g = _part_args(field, n, kind, cs_degree, last_row, theta, beta, gamma, y, fixed, advice, instance,
                            challenges, l_first, l_last, l_active_row, graph, graph2, z, a_perm, s_perm, perm_columns,
                            sigmas, x_scale, omega, delta)
    if _is_cuda(acc):
        ptr, nb, k = _ptr(acc)
        a.hold(k)
        buf = None
    else:
        buf = ctypes.create_string_buffer(bytes(acc), max(1, 32 * n))
        ptr, nb = ctypes.addressof(buf), len(bytes(acc))
    if nb != 32 * n:
        raise ValueError("acc: n 32-byte elements")
    a.sync()
    ok = lib().tachyon_mi355x_quotient_evaluate_part(ctypes.byref(p), ctypes.byref(t), ctypes.byref(g), ptr)
    if not ok:
        return None
    return acc if buf is None else buf.raw[:32 * n]


def quotient_program_stats(field, n, kind, *, cs_degree=3, last_row=0, theta, beta, gamma, y, fixed=(), advice=(),
                           instance=(), challenges=(), l_first=None, l_last=None, l_active_row=None, graph=None,
                           graph2=None, z=(), a_perm=None, s_perm=None, perm_columns=(), sigmas=(), x_scale=None,
                           omega=None, delta=None):
    """tachyon_mi355x_quotient_program_stats: the lowered program of the group
    quotient_evaluate_part would run, on the host alone -- a dict of its
    instructions, products (Mul and Square), column_reads per row and
    slots_needed; None for a group the call refuses."""
    a, p, t, g = _part_args(field, n, kind, cs_degree, last_row, theta, beta, gamma, y, fixed, advice, instance,
                            challenges, l_first, l_last, l_active_row, graph, graph2, z, a_perm, s_perm, perm_columns,
                            sigmas, x_scale, omega, delta)
    out = (ctypes.c_size_t * 4)()
    if not lib().tachyon_mi355x_quotient_program_stats(ctypes.byref(p), ctypes.byref(t), ctypes.byref(g), out):
        return None
    return dict(zip(("instructions", "products", "column_reads", "slots_needed"), [int(x) for x in out]))


def _system(a, gates, perm_columns, sigmas, lookups, shuffles):
    s = QSystem()
    s.gates = a.graph(gates)
    s.perm_columns, s.num_perm_columns = a.sources(list(perm_columns)), len(perm_columns)
    s.sigmas = a.columns(list(sigmas))
    s.lookups, s.num_lookups = a.graphs(list(lookups)), len(lookups)
    s.shuffles, s.num_shuffles = a.graphs([g for pair in shuffles for g in pair]), len(shuffles)
    return s


def _circuits(a, circuits):
    arr = (QCircuit * max(1, len(circuits)))()
    for c, src in zip(arr, circuits):
        a.table(c.table, list(src.get("fixed", ())), list(src.get("advice", ())), list(src.get("instance", ())),
                list(src.get("challenges", ())))
        pz = list(src.get("perm_z", ()))
        c.perm_z, c.num_perm_z = a.columns(pz), len(pz)
        lk = list(src.get("lookups", ()))  # (Z, A', S') per lookup
        c.lookup_z = a.columns([x[0] for x in lk])
        c.lookup_a_perm = a.columns([x[1] for x in lk])
        c.lookup_s_perm = a.columns([x[2] for x in lk])
        c.shuffle_z = a.columns(list(src.get("shuffle_z", ())))
    a.keep.append(arr)
    return arr


def _h_args(field, n, cs_degree, last_row, theta, beta, gamma, y, l_first, l_last, l_active_row, gates, perm_columns,
            sigmas, lookups, shuffles, circuits):
    a = _Args(field, n)
    p = a.params(cs_degree, last_row, theta, beta, gamma, y, l_first, l_last, l_active_row)
    s = _system(a, gates, perm_columns, sigmas, lookups, shuffles)
    return a, p, s, _circuits(a, circuits)


def quotient_work_bytes(field, n, circuits, *, cs_degree, last_row=0, theta, beta, gamma, y, l_first, l_last,
                        l_active_row, gates=None, perm_columns=(), sigmas=(), lookups=(), shuffles=()) -> int:
    """tachyon_mi355x_quotient_work_bytes: an upper bound of the device memory
    quotient_h_poly of this shape holds, before anything is allocated; 0 for
    a shape the call refuses."""
    a, p, s, c = _h_args(field, n, cs_degree, last_row, theta, beta, gamma, y, l_first, l_last, l_active_row, gates,
                         perm_columns, sigmas, lookups, shuffles, circuits)
    return lib().tachyon_mi355x_quotient_work_bytes(ctypes.byref(p), ctypes.byref(s), c, len(circuits))


def quotient_h_poly(field, n, circuits, *, cs_degree, last_row=0, theta, beta, gamma, y, zeta, delta=None, l_first,
                    l_last, l_active_row, gates=None, perm_columns=(), sigmas=(), lookups=(), shuffles=(),
                    ext_gen=None, full=False, out=None):
    """tachyon_mi355x_quotient_h_poly: h(X) from coefficient-form polynomials.
    circuits: per circuit a dict {fixed, advice, instance, challenges, perm_z,
    lookups: [(Z, A', S')], shuffle_z}; gates / lookups: GraphEvaluators;
    shuffles: (input, shuffle) GraphEvaluator pairs; perm_columns: (kind,
    index) pairs; ext_gen: the extended domain's generator (None: the
    field's root of the active generator set); out: a CUDA tensor for the
    n (cs_degree - 1) coefficients (n 2^(extended_k - k) with full), else bytes
    are returned.  None on a refusal."""
    a, p, s, c = _h_args(field, n, cs_degree, last_row, theta, beta, gamma, y, l_first, l_last, l_active_row, gates,
                         perm_columns, sigmas, lookups, shuffles, circuits)
    count = (n << (extended_k(n, cs_degree) - (n.bit_length() - 1))) if full else n * (cs_degree - 1)
    if out is None:
        buf = ctypes.create_string_buffer(max(1, 32 * count))
        ptr = ctypes.addressof(buf)
    else:
        ptr, nb, k = _ptr(out)
        if nb != 32 * count:
            raise ValueError("out: 32 bytes per coefficient")
        a.hold(k)
    a.sync()
    ok = lib().tachyon_mi355x_quotient_h_poly(ctypes.byref(p), ctypes.byref(s), c, len(circuits), a.elem(zeta),
                                              a.elem(delta), a.elem(ext_gen), 1 if full else 0, ptr)
    if not ok:
        return None
    return out if out is not None else buf.raw[:32 * count]
