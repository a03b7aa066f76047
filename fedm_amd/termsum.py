"""Normal form of field-dependent coefficients:  f(E) = sum_i c_i E^p_i exp(q_i E^r_i).

The streamer deck gives mobility, diffusion and ionisation coefficients as
one-line Python/UFL strings in ``E_m`` (the magnitude of the electric field),
e.g. ``2.3987*E_m**(-0.26)`` (transport_coefficients/e_Nb.dat:12) or
``(1.1944e6 + 4.3666e26 * E_m**(-3))*exp(-2.73e7/E_m)-340.75`` (alpha.dat:12),
which the reference ``eval``s into UFL (fedm-streamer.py:237-239).  Here the
string is parsed with a restricted ``ast`` grammar (never ``eval``) and
expanded into a sum of generalised monomials, which the element kernel
evaluates -- value and d/dE -- once per cell.

Coefficients that come as two-column tables against E/N (the decks'
``Dependence: E/N`` files, Boltzmann-solver output) multiply such a sum by up
to two piecewise-linear table factors:  f(E) = g(E) * T1(E) [* T2(E)], with
np.interp's value and the exact derivative (the segment's slope between the
first and the last knot, 0 outside).  The element kernel looks them up at the
cell's own |E|; see ``TermSum.table``.
"""
import ast
import math
from numbers import Real

import numpy as np

MAX_TABLE_FACTORS = 2


class Table:
    """Piecewise-linear T(E): knots x [V/m] strictly increasing, values y, constant outside the knots."""

    def __init__(self, x, y):
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        self.y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if self.x.size < 1 or self.x.size != self.y.size:
            raise ValueError("a coefficient table needs as many values as knots, and at least one")
        if not (np.isfinite(self.x).all() and np.isfinite(self.y).all()):
            raise ValueError("a coefficient table's knots and values must be finite")
        if np.any(np.diff(self.x) <= 0.0):
            raise ValueError("a coefficient table's knots must strictly increase")

    def key(self):
        return self.x.tobytes(), self.y.tobytes()

    def __call__(self, E):
        return float(np.interp(E, self.x, self.y))

    def derivative(self, E):
        x, y = self.x, self.y
        if E != E:
            return float("nan")
        if x.size < 2 or not (x[0] <= E < x[-1]):
            return 0.0
        j = min(max(int(np.searchsorted(x, E, side="right")) - 1, 0), x.size - 2)
        return float((y[j + 1] - y[j]) / (x[j + 1] - x[j]))

    def scaled(self, c):
        return Table(self.x, c * self.y)


class TermSum:
    __array_priority__ = 1000

    def __init__(self, terms=(), tables=()):
        self.tables = tuple(tables)
        merged = {}
        for c, p, q, r in terms:
            c, p, q, r = float(c), float(p), float(q), float(r)
            if q == 0.0:
                r = 0.0
            key = (p, q, r)
            merged[key] = merged.get(key, 0.0) + c
        self.terms = [(c, p, q, r) for (p, q, r), c in merged.items() if c != 0.0]
        if not self.terms:               # the zero coefficient: no look-up, and no factor that counts towards the limit
            self.tables = ()
        if len(self.tables) > MAX_TABLE_FACTORS:
            raise ValueError(f"product of {len(self.tables)} tabulated coefficients: a coefficient takes at most "
                             f"{MAX_TABLE_FACTORS} table factors")

    # -- constructors ---------------------------------------------------------
    @classmethod
    def const(cls, c):
        return cls([(float(c), 0.0, 0.0, 0.0)])

    @classmethod
    def field(cls):
        """The symbol E_m itself."""
        return cls([(1.0, 1.0, 0.0, 0.0)])

    @classmethod
    def table(cls, x_E, y):
        """The tabulated coefficient T(|E|): knots ``x_E`` in V/m (E/N in Td times N0 * 1e-21), values ``y``."""
        return cls([(1.0, 0.0, 0.0, 0.0)], tables=(Table(x_E, y),))

    @classmethod
    def coerce(cls, v):
        if isinstance(v, TermSum):
            return v
        if isinstance(v, Real):
            return cls.const(v)
        if isinstance(v, str):
            return parse(v)
        raise TypeError(f"cannot interpret {v!r} as a coefficient of |E|")

    # -- queries ----------------------------------------------------------------
    def is_const(self):
        return not (self.tables and self.terms) and all(p == 0.0 and q == 0.0 for _, p, q, _ in self.terms)

    def same_as(self, o):
        """The same function of |E|, term by term and table by table (in whatever order the factors were multiplied)."""
        return self.terms == o.terms and sorted(t.key() for t in self.tables) == sorted(t.key() for t in o.tables)

    def const_value(self):
        if not self.is_const():
            raise ValueError("coefficient depends on |E|")
        return sum(c for c, *_ in self.terms)

    def _g(self, E):
        return sum(c * E ** p * math.exp(q * E ** r if q else 0.0) for c, p, q, r in self.terms)

    def _dg(self, E):
        return sum(c * E ** p * math.exp(q * E ** r if q else 0.0) * (p + r * q * E ** r) / E
                   for c, p, q, r in self.terms if (p or q))

    def __call__(self, E):
        val = self._g(E)
        for t in self.tables:
            val = val * t(E)
        return val

    def derivative(self, E):
        val, der = self._g(E), self._dg(E)
        for t in self.tables:            # the product rule, factor by factor (as the element kernel does)
            tv, td = t(E), t.derivative(E)
            val, der = val * tv, der * tv + val * td
        return der

    def fill(self, cstruct, tables=None):
        """Write the coefficient into a ``fedm_termsum``.  ``tables``: the list of the model's distinct
        :class:`Table` objects, extended here (equal arrays go in once); the struct's table reference holds
        1 + index of the first factor in its low and of the second in its high 16 bits."""
        from . import _lib
        if len(self.terms) > _lib.MAX_TERMS:
            raise ValueError(f"coefficient has {len(self.terms)} terms, at most {_lib.MAX_TERMS}")
        cstruct.n_terms = len(self.terms)
        for i, (c, p, q, r) in enumerate(self.terms):
            # (+ 0.0: a negative zero left by the algebra becomes +0.0 -- the same model, the same bytes)
            cstruct.c[i], cstruct.p[i], cstruct.q[i], cstruct.r[i] = c + 0.0, p + 0.0, q + 0.0, r + 0.0
        ref = 0
        if self.tables and self.terms:   # (a zero coefficient needs no look-up)
            if tables is None:
                raise ValueError("a tabulated coefficient is written together with the model's tables: "
                                 "Model.to_c_tabulated()")
            for k, t in enumerate(self.tables):
                keys = [u.key() for u in tables]
                if t.key() in keys:
                    idx = keys.index(t.key())
                else:
                    if len(tables) >= _lib.MAX_TABLES:
                        raise ValueError(f"model has more than {_lib.MAX_TABLES} distinct coefficient tables")
                    tables.append(t)
                    idx = len(tables) - 1
                ref |= (idx + 1) << (16 * k)
        cstruct.pad_ = ref

    # -- algebra ------------------------------------------------------------------
    def _one_table_form(self):
        """(constant, Table or None) when the coefficient is constant * one table, or a constant; else None."""
        if len(self.tables) > 1 or any(p != 0.0 or q != 0.0 for _, p, q, _ in self.terms):
            return None
        c = sum(c for c, *_ in self.terms)
        return (c, self.tables[0]) if self.tables and self.terms else (c, None)

    def __add__(self, o):
        o = TermSum.coerce(o)
        if not self.tables and not o.tables:
            return TermSum(self.terms + o.terms)
        if not self.terms:               # 0 + f
            return o
        if not o.terms:
            return self
        a, b = self._one_table_form(), o._one_table_form()
        if a is None or b is None:
            raise ValueError("sum with a tabulated coefficient: only constant * table (+ constant * table, or + "
                             "constant) can be added -- exactly, on the union of the knots; not a table times a "
                             "function of |E| or a product of tables")
        # a sum of clamped piecewise-linear functions is piecewise linear on the union grid, clamped at its ends
        x = np.unique(np.concatenate([t.x for _, t in (a, b) if t is not None]))
        y = np.zeros_like(x)
        for c, t in (a, b):
            y = y + (c * np.interp(x, t.x, t.y) if t is not None else c)
        return TermSum.table(x, y)

    __radd__ = __add__

    def __neg__(self):
        return TermSum([(-c, p, q, r) for c, p, q, r in self.terms], self.tables)

    def __sub__(self, o):
        return self + (-TermSum.coerce(o))

    def __rsub__(self, o):
        return TermSum.coerce(o) - self

    def __mul__(self, o):
        if not isinstance(o, (TermSum, Real)):
            return NotImplemented
        o = TermSum.coerce(o)
        out = []
        for c1, p1, q1, r1 in self.terms:
            for c2, p2, q2, r2 in o.terms:
                if q1 == 0.0:
                    q, r = q2, r2
                elif q2 == 0.0:
                    q, r = q1, r1
                elif r1 == r2:
                    q, r = q1 + q2, r1
                else:
                    raise ValueError("product of exponentials with different powers of |E| "
                                     "is outside the supported coefficient family")
                out.append((c1 * c2, p1 + p2, q, r))
        return TermSum(out, self.tables + o.tables)

    __rmul__ = __mul__

    def __pow__(self, n):
        if isinstance(n, TermSum):
            n = n.const_value()
        n = float(n)
        if self.tables and self.terms:
            if n == 1.0:
                return self
            raise ValueError("power (or reciprocal) of a tabulated coefficient is outside the supported "
                             "coefficient family: tabulate the power itself")
        if len(self.terms) == 1:
            c, p, q, r = self.terms[0]
            return TermSum([(c ** n, p * n, q * n, r)])
        if n == int(n) and n >= 0:
            out = TermSum.const(1.0)
            for _ in range(int(n)):
                out = out * self
            return out
        raise ValueError("non-integer power of a sum is outside the supported coefficient family")

    def __truediv__(self, o):
        return self * TermSum.coerce(o) ** -1.0

    def __rtruediv__(self, o):
        return TermSum.coerce(o) * self ** -1.0

    def exp(self):
        """exp of a constant or of a single monomial a*E^b."""
        if not self.terms:
            return TermSum.const(1.0)
        if self.tables:
            raise ValueError("exp() of a tabulated coefficient is outside the supported coefficient family: "
                             "tabulate the exponential itself")
        const = sum(c for c, p, q, _ in self.terms if p == 0.0 and q == 0.0)
        rest = [(c, p, q, r) for c, p, q, r in self.terms if not (p == 0.0 and q == 0.0)]
        if len(rest) > 1 or any(q != 0.0 for _, _, q, _ in rest):
            raise ValueError("exp() argument must be a*E_m**b (+ constant)")
        if not rest:
            return TermSum.const(math.exp(const))
        c, p, _, _ = rest[0]
        return TermSum([(math.exp(const), 0.0, c, p)])

    def __repr__(self):
        return "TermSum(" + " + ".join(
            f"{c:g}*E^{p:g}" + (f"*exp({q:g}*E^{r:g})" if q else "") for c, p, q, r in self.terms) + ")" + "".join(
            f"*Table({t.x.size} knots)" for t in self.tables)


_BINOPS = {ast.Add: lambda a, b: a + b, ast.Sub: lambda a, b: a - b,
           ast.Mult: lambda a, b: a * b, ast.Div: lambda a, b: a / b,
           ast.Pow: lambda a, b: a ** b}


def parse(text, symbol="E_m"):
    """Parse a deck expression in ``E_m`` into a :class:`TermSum` (no eval)."""
    try:
        tree = ast.parse(text.strip(), mode="eval")
    except SyntaxError as exc:
        raise ValueError(f"cannot parse coefficient expression {text!r}") from exc

    def walk(node):
        if isinstance(node, ast.Expression):
            return walk(node.body)
        if isinstance(node, ast.Constant) and isinstance(node.value, (int, float)):
            return TermSum.const(node.value)
        if isinstance(node, ast.Name):
            if node.id == symbol:
                return TermSum.field()
            if node.id == "pi":
                return TermSum.const(math.pi)
            raise ValueError(f"unknown symbol {node.id!r} in coefficient expression {text!r}")
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, (ast.USub, ast.UAdd)):
            v = walk(node.operand)
            return -v if isinstance(node.op, ast.USub) else v
        if isinstance(node, ast.BinOp) and type(node.op) in _BINOPS:
            return _BINOPS[type(node.op)](walk(node.left), walk(node.right))
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and not node.keywords:
            args = [walk(a) for a in node.args]
            if node.func.id == "exp" and len(args) == 1:
                return args[0].exp()
            if node.func.id == "sqrt" and len(args) == 1:
                return args[0] ** 0.5
            if node.func.id == "pow" and len(args) == 2:
                return args[0] ** args[1]
        raise ValueError(f"unsupported construct in coefficient expression {text!r}")

    return walk(tree)
