"""Tabulated E/N coefficients for the oracle and the models of the tabulated-coefficient tests (helper module).

oracle/forms.py evaluates a coefficient as ``m(Em) -> (value, derivative)`` and leaves an instance of its own TermSum
class alone, so a subclass that multiplies table factors on plugs into LFAModel and oracle.newton unchanged.  The
look-up semantics are those of fedm_amd/csrc/table_lookup.h, restated with numpy: np.interp's value; the segment's
slope for x[0] <= E < x[n-1], exactly 0 outside and for one knot.
"""
import numpy as np

from oracle.forms import TermSum as OTermSum


def table_eval(x, y, E):
    """(value, derivative) of the piecewise-linear table at E (array)."""
    x, y, E = np.asarray(x, float), np.asarray(y, float), np.asarray(E, float)
    val = np.interp(E, x, y)
    der = np.zeros_like(E)
    if x.size >= 2:
        slope = np.diff(y) / np.diff(x)
        j = np.clip(np.searchsorted(x, E, side="right") - 1, 0, x.size - 2)
        inside = (E >= x[0]) & (E < x[-1])
        der = np.where(inside, slope[j], 0.0)
    nan = np.isnan(E)
    return np.where(nan, np.nan, val), np.where(nan, np.nan, der)


class TabulatedTermSum(OTermSum):
    """g(E) * T1(E) [* T2(E)]: an oracle term sum times piecewise-linear tables (x [V/m], y)."""

    def __init__(self, terms, tables):
        super().__init__(terms)
        self.tables = [(np.asarray(x, float), np.asarray(y, float)) for x, y in tables]

    def __call__(self, E):
        val, der = super().__call__(E)
        for x, y in self.tables:
            tv, td = table_eval(x, y, E)
            val, der = val * tv, der * tv + val * td
        return val, der


def quantile_knots(Em, n=9, lo=0.10, hi=0.90):
    """n log-spaced knots between two quantiles of the cells' |E|: both clamped regions and the segments between
    are populated by construction."""
    a, b = np.quantile(Em, [lo, hi])
    return np.geomspace(a, b, n)


def assert_knots_exercise_the_lookup(x, Em, min_segments=3):
    """Precondition of a comparison between two implementations, not a filter: both clamped regions and several
    segments hold cells, and no cell sits within 1e-9 relative of a knot (at a kink two correct implementations may
    pick different slopes).  No cell is excluded from anything."""
    x = np.asarray(x, float)
    assert (Em < x[0]).sum() > 0 and (Em > x[-1]).sum() > 0
    seg = np.searchsorted(x, Em[(Em >= x[0]) & (Em < x[-1])], side="right") - 1
    assert np.unique(seg).size >= min(min_segments, x.size - 1)
    assert (np.abs(Em[:, None] - x[None, :]) / x[None, :]).min() > 1e-9


def closed_forms(x):
    """mu_e, D_e and alpha of the benchmark deck (oracle/streamer.py's numbers) at the knots x."""
    x = np.asarray(x, float)
    mu = 2.3987 * x ** -0.26
    D = 4.3628e-3 * x ** 0.22
    alpha = (1.1944e6 + 4.3666e26 * x ** -3.0) * np.exp(-2.73e7 / x) - 340.75
    return mu, D, alpha


def oracle_streamer(mesh, x):
    """The oracle's streamer model with mu_e and D_e tabulated and k = T_alpha * T_mu * E (two table factors)."""
    from oracle import streamer as ost
    om = ost.build(mesh)
    mu, D, alpha = closed_forms(x)
    one = [(1.0, 0.0, 0.0, 0.0)]
    om.mu[1] = TabulatedTermSum(one, [(x, mu)])
    om.D[1] = TabulatedTermSum(one, [(x, D)])
    k = TabulatedTermSum([(1.0, 1.0, 0.0, 0.0)], [(x, alpha), (x, mu)])
    om.reactions = [(k, P, nu) for _, P, nu in om.reactions]
    return om


def device_streamer_model(x):
    """The same model for the device: fedm_amd.device.Model with TermSum.table coefficients."""
    from fedm_amd.cases import streamer
    from fedm_amd.device import Model, Reaction
    from fedm_amd.termsum import TermSum
    mu_y, D_y, alpha_y = closed_forms(x)
    mu = TermSum.table(x, mu_y)
    rate = TermSum.table(x, alpha_y) * mu * TermSum.field()
    return Model(n_species=2, poisson=True, eq_type=["reaction", "drift-diffusion-reaction"], Z=[1.0, -1.0],
                 mu=[TermSum.const(0.0), mu], D=[TermSum.const(0.0), TermSum.table(x, D_y)],
                 reactions=[Reaction(rate, power=[0, 1], net=[1, 1])], bc_kind=streamer.BC_TYPE, quadrature_degree=2)


def device_streamer_problem(coords, cells, model):
    from fedm_amd.cases import streamer
    from fedm_amd.device import DeviceProblem
    from fedm_amd.mesh import Marking_boundaries, Mesh
    msh = Mesh(coords, cells)
    dofs, vals = streamer.dirichlet(msh.coords)
    return DeviceProblem(msh.coords, msh.cells, model, facet_tags=Marking_boundaries(msh, streamer.BOUNDARIES),
                         dirichlet_dofs=dofs, dirichlet_vals=vals)


def oracle_coefficient(ts):
    """A fedm_amd TermSum (with or without table factors) as the oracle's coefficient: the same numbers."""
    return TabulatedTermSum(ts.terms, [(t.x, t.y) for t in ts.tables])


def oracle_model_of(mesh, model):
    """The oracle's streamer model with the coefficients of a two-species device Model (cases/streamer.py's shape)."""
    from oracle import streamer as ost
    om = ost.build(mesh)
    om.mu[1], om.D[1] = oracle_coefficient(model.mu[1]), oracle_coefficient(model.D[1])
    om.reactions = [(oracle_coefficient(model.reactions[0].k), P, nu) for _, P, nu in om.reactions]
    return om
