"""The postfix interpreter of ``Expression`` sources (csrc/gdprep.hip: ext_source_eval_kernel) and the source tables in
the assembly, beyond the one program, degree and mesh that test_gpu_parity.py runs: every opcode, the lattices of
degree 1, 2 and 3 (3, 6 and 10 nodes a cell, the kernel's own walk over the rows of the lattice), the stack limit, all
16 parameters, ``ext_B`` with 3 and 10 columns against the oracle, two species with tables of their own, a Delaunay
mesh with a non-trivial vertex reordering.  The tables are read back with ``DeviceProblem.get_ext_source``.

Meshes: a structured 6x8 mesh of [0.5, 1.5] x [0.5, 2] and a graded Delaunay mesh of the same box (coordinates of
order one: well-conditioned arguments for every function); for the time-of-flight source, whose pulse lives in a box
of 0.25 mm x 0.5 mm, a 12x12 mesh and a graded Delaunay mesh of that box.

Tolerances:
* node coordinates: 4 eps relative -- three products and two sums, possibly fused.
* values: 32 eps |ref| + the change of the reference when each coordinate moves by 4 ulp.  The device's math library
  aims at the OpenCL double-precision bounds, of which pow's 16 ulp is the largest; 32 eps leaves a factor two for the
  arithmetic around the call.  MEASURED on the MI355X, worst |dev - ref| / (eps |ref|) over the entries with
  |ref| > 0.1 of each opcode's program: against the reference nodes | against the host interpreter run at the
  coordinates the DEVICE computed (the interpreter's and the math library's own error):
      const 0.00 | 0.00   x    1.29 | 0.00   param 0.00 | 0.00   add   0.99 | 0.00   sub  6.75 | 0.00   mul  3.01 | 0.00
      div   1.69 | 0.00   pow  1.99 | 1.00   neg   1.29 | 0.00   exp   2.61 | 1.00   log 14.41 | 0.99   sqrt 0.99 | 0.00
      sin  31.79 | 0.88   cos 14.59 | 0.97   tan   2.86 | 0.96   fabs  9.60 | 0.00   tanh 6.98 | 0.95   atan 6.73 | 0.83
  The arithmetic opcodes and sqrt are bit-equal to the host at equal coordinates; every library function stayed
  within 1 eps of numpy's there, pow (16 ulp by the library's specification) included: no opcode came near the
  library bound.  The large figures of the first column are the coordinates' 1.3 eps through an ill-conditioned argument
  (sin(3 x) next to a root, log next to 1, a difference next to its zero), which the second term of the tolerance
  carries: no program used more than 0.33 of its tolerance (sin; cos 0.31, atan 0.24).
* residual and Jacobian against the oracle: 1e-11 and 1e-10, as in test_gpu_unstructured.py.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import scipy.sparse as sp

sys.path.insert(0, str(Path(__file__).resolve().parent))

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NODES = {1: 3, 2: 6, 3: 10}


def _unit_meshes():
    from fedm_amd import meshgen
    from fedm_amd.mesh import Mesh, RectangleMesh
    size = meshgen.box_distance_size((0.0, 1.0, 0.0, 0.2), 0.04, 0.4, 0.3)
    graded = meshgen.refined_rectangle(1.0, 1.5, size, 0.04, n_levels=4)
    return {"structured": RectangleMesh((0.5, 0.5), (1.5, 2.0), 6, 8),
            "delaunay": Mesh(graded.coords + 0.5, graded.cells)}


def _tof_meshes():
    from fedm_amd import meshgen
    from fedm_amd.mesh import RectangleMesh
    size = meshgen.box_distance_size((0.0, 0.6e-4, 3.5e-4, 5e-4), 4e-6, 0.25, 4e-5)      # fine around the pulse
    return {"structured": RectangleMesh((0.0, 0.0), (2.5e-4, 5e-4), 12, 12),
            "delaunay": meshgen.refined_rectangle(2.5e-4, 5e-4, size, 4e-6, n_levels=4)}


def _model(degrees, **kw):
    from fedm_amd.device import Model
    from fedm_amd.termsum import TermSum
    ns = len(degrees)
    args = dict(n_species=ns, poisson=False, eq_type=["drift-diffusion-reaction"] * ns, Z=[-1.0] * ns,
                D=[TermSum.const(d) for d in (0.12, 0.05)[:ns]], drift_w=[(0.0, 1.7), (0.3, -0.5)][:ns],
                quadrature_degree=8, ext_source_degree=list(degrees))
    args.update(kw)
    return Model(**args)


@pytest.fixture(scope="module")
def unit():
    """{(mesh name, degree): (mesh, oracle mesh, one-species device problem)} on the order-one box."""
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.device import DeviceProblem
    out = {}
    for name, m in _unit_meshes().items():
        for k in NODES:
            out[name, k] = (m, OMesh(m.coords, m.cells), DeviceProblem(m.coords, m.cells, _model([k])))
    assert out["structured", 2][0].num_vertices() == 63
    # the Delaunay mesh is renumbered inside the device problem, nearly every vertex moves
    prob = out["delaunay", 2][2]
    assert (prob._order != np.arange(prob.nv)).sum() > prob.nv // 2
    yield out
    for _, _, prob in out.values():
        prob.close()


def _run(prob, species, text, **params):
    """The string as a device program, evaluated with its parameters: (table read back, ops, consts, values)."""
    from fedm_amd import forms
    f = forms.Expression(text, degree=2, **params)
    ops, consts, names = forms.expression_program(f)
    prob.set_ext_source_program(species, ops, consts, len(names))
    values = [float(getattr(f, n)) for n in names]
    prob.eval_ext_source(species, values)
    return prob.get_ext_source(species), ops, consts, values


def _tolerance(ops, consts, values, nodes):
    """32 eps |ref| + what 4 ulp of each coordinate do to the reference."""
    from fedm_amd import forms
    want = forms.run_expression_program(ops, consts, values, nodes)
    moved = np.zeros_like(want)
    for c in (0, 1):
        worst = np.zeros_like(want)
        for sign in (-1.0, 1.0):
            x = nodes.copy()
            x[..., c] *= 1.0 + sign * 4.0 * EPS
            worst = np.maximum(worst, np.abs(forms.run_expression_program(ops, consts, values, x) - want))
        moved += worst
    return want, 32.0 * EPS * np.abs(want) + moved


# ---- lattice order --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["structured", "delaunay"])
def test_lattice_nodes_in_the_oracles_order(unit, name, k):
    """x[0] and x[1] as programs: the table IS the node coordinates -- a wrong walk over the lattice rows, a turned
    cell or another cell order shows at once."""
    from oracle import tof as otof
    m, om, prob = unit[name, k]
    nodes = otof.cell_nodes(om, k)
    assert nodes.shape == (m.cells.shape[0], NODES[k], 2)
    assert len({tuple(p) for p in np.round(nodes[0] / 1e-9)}) == NODES[k]          # distinct nodes
    for c in (0, 1):
        table, _, _, _ = _run(prob, 0, f"x[{c}]")
        assert table.shape == (m.cells.shape[0], NODES[k])
        assert (np.abs(table - nodes[..., c]) <= 4.0 * EPS * np.abs(nodes[..., c])).all()


# ---- every opcode ---------------------------------------------------------------------------------------------------
PROGRAMS = {      # opcode: (string, parameters); operands from constants, coordinates and parameters
    "const": ("2.5", {}),
    "x": ("x[1]", {}),
    "param": ("a", dict(a=1.75)),
    "add": ("x[0]+a", dict(a=0.375)),
    "sub": ("a-x[1]", dict(a=0.7)),
    "mul": ("0.3*x[0]*x[1]", {}),
    "div": ("a/x[1]", dict(a=1.3)),
    "pow": ("pow(x[0], 1.5)", {}),
    "neg": ("-x[1]", {}),
    "exp": ("exp(-a*x[0])", dict(a=2.2)),
    "log": ("log(x[0]*x[1])", {}),
    "sqrt": ("sqrt(x[0]+a)", dict(a=0.1)),
    "sin": ("sin(3.0*x[1])", {}),
    "cos": ("cos(a*x[0])", dict(a=2.0)),
    "tan": ("tan(0.3*x[0])", {}),
    "fabs": ("fabs(x[0]-1.0)", {}),
    "tanh": ("tanh(x[1]-a)", dict(a=1.2)),
    "atan": ("atan(x[1]-1.0)", {}),
}


@pytest.mark.parametrize("opcode", list(PROGRAMS))
def test_every_opcode_against_the_host_interpreter(unit, opcode):
    from oracle import tof as otof
    from fedm_amd import _lib, forms
    assert set(PROGRAMS) == set(_lib.EXPR_OPS) - {"abs"} and len(PROGRAMS) == 18
    text, params = PROGRAMS[opcode]
    worst = share = own = 0.0
    for name, k in (("structured", 2), ("delaunay", 3), ("delaunay", 1)):
        m, om, prob = unit[name, k]
        table, ops, consts, values = _run(prob, 0, text, **params)
        assert _lib.EXPR_OPS[opcode] in ops[:, 0]
        want, tol = _tolerance(ops, consts, values, otof.cell_nodes(om, k))
        assert np.isfinite(want).all() and np.abs(want).max() > 0.1
        err = np.abs(table - want)
        big = np.abs(want) > 0.1                          # (relative figures mean little next to a zero of the function)
        worst = max(worst, float(np.max(err[big] / (EPS * np.abs(want[big])))))
        share = max(share, float(np.max(err / np.maximum(tol, 1e-300))))
        assert (err <= tol).all(), f"{opcode}: {share:.2f} of its tolerance"
        # the interpreter's own error: against the host interpreter at the coordinates the DEVICE computed
        here = np.stack([_run(prob, 0, "x[0]")[0], _run(prob, 0, "x[1]")[0]], axis=-1)
        same = forms.run_expression_program(ops, consts, values, here)
        own = max(own, float(np.max(np.abs(table - same)[big] / (EPS * np.abs(same[big])))))
    print(f"opcode {opcode} ({text}): {share:.3f} of the tolerance; worst {worst:.2f} eps |ref| where |ref| > 0.1, "
          f"{own:.2f} eps at the device's own coordinates")


# ---- limits ---------------------------------------------------------------------------------------------------------
def test_stack_depth_24_runs_and_25_is_refused(unit):
    from oracle import tof as otof
    from fedm_amd import _lib, forms
    assert _lib.EXPR_STACK == 24
    m, om, prob = unit["delaunay", 2]
    nodes = otof.cell_nodes(om, 2)

    def nested(n):                                     # t1+(t2+(...+tn)): n operands on the stack before the first add
        terms = [f"x[{i % 2}]" if i % 3 else f"{0.25 * (i + 1)}" for i in range(n)]
        return "+(".join(terms) + ")" * (n - 1)

    table, ops, consts, values = _run(prob, 0, nested(24))
    depth = np.cumsum(np.where(ops[:, 0] <= 2, 1, np.where(ops[:, 0] <= 7, -1, 0)))
    assert depth.max() == 24 and depth[-1] == 1
    want, tol = _tolerance(ops, consts, values, nodes)
    assert (np.abs(table - want) <= tol).all()
    with pytest.raises(NotImplementedError, match="too long"):
        forms.expression_program(forms.Expression(nested(25), degree=2))
    deep = [[1, 0]] * 25 + [[3, 0]] * 24                 # the same program handed to the library directly
    with pytest.raises(RuntimeError, match="bad expression program"):
        prob.set_ext_source_program(0, deep, [], 0)
    # the refusal left the installed program alone
    prob.eval_ext_source(0, [])
    assert np.array_equal(prob.get_ext_source(0), table)


def test_sixteen_parameters_and_a_table_replaced_as_a_whole(unit):
    from oracle import tof as otof
    from fedm_amd import _lib, forms
    assert _lib.EXPR_MAX_PARAMS == 16
    m, om, prob = unit["structured", 3]
    nodes = otof.cell_nodes(om, 3)
    text = "+".join(f"p{i}*x[{i % 2}]" if i % 4 else f"p{i}" for i in range(16))
    first = {f"p{i}": 0.5 + 0.125 * i for i in range(16)}
    table, ops, consts, values = _run(prob, 0, text, **first)
    assert len(values) == 16 and values == list(first.values())
    want, tol = _tolerance(ops, consts, values, nodes)
    assert (np.abs(table - want) <= tol).all()
    second = [(-1.0) ** i * (3.0 - 0.17 * i) for i in range(16)]
    prob.eval_ext_source(0, second)
    again = prob.get_ext_source(0)
    want2, tol2 = _tolerance(ops, consts, second, nodes)
    assert (np.abs(again - want2) <= tol2).all()
    assert (again != table).all()                      # every entry is new
    with pytest.raises(NotImplementedError, match="too long"):
        forms.expression_program(forms.Expression(text + "+p16", degree=2, p16=1.0, **first))


# ---- degrees 1 and 3 through the assembly ---------------------------------------------------------------------------
def _rel_rows(A, B):
    D = abs(A - B)
    scale = np.maximum(abs(B).max(axis=1).toarray().ravel(), 1e-300)
    return (sp.diags(1.0 / scale) @ D).max()


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("name", ["structured", "delaunay"])
def test_time_of_flight_source_of_degree_1_and_3_in_residual_and_jacobian(name, k):
    """ext_B with 3 and 10 columns: the time-of-flight source string at degree k, once as a table computed on the host
    and uploaded, once evaluated by the device, in the residual and the Jacobian against the oracle."""
    from oracle import tof as otof
    from oracle.forms import LFAModel
    from oracle.mesh import Mesh as OMesh
    from fedm_amd import forms
    from fedm_amd.cases import time_of_flight as tof
    from fedm_amd.device import DeviceProblem, Model
    from fedm_amd.termsum import TermSum
    m = _tof_meshes()[name]
    om = OMesh(m.coords, m.cells)
    prob = DeviceProblem(m.coords, m.cells, Model(n_species=1, poisson=False, eq_type=["drift-diffusion-reaction"],
                                                  Z=[-1.0], D=[TermSum.const(tof.DE)], drift_w=[(0.0, tof.WEZ)],
                                                  quadrature_degree=8, ext_source_degree=[k]))
    o = LFAModel(om, 1, False, ["drift-diffusion-reaction"], [-1.0], D=[otof.DE], drift_w=[(0.0, otof.WEZ)], qdeg=8)
    t0, dt, dt_old = 2.5e-9, 1e-12, 2e-12
    rng = np.random.default_rng(k)
    U = otof.log_density(om.coords, t0, 3e-16)[:, None] + rng.normal(0, 0.1, (om.nv, 1))
    Uo = otof.log_density(om.coords, t0)[:, None]
    Uo1 = Uo + rng.normal(0, 0.1, (om.nv, 1))
    nodes = otof.cell_nodes(om, k)
    o.set_ext_source(0, k, otof.source(nodes, t0 + dt))
    F_cpu, J_cpu = o.residual_jacobian(U, Uo, Uo1, dt, dt_old)
    o.set_ext_source(0, k, np.zeros(nodes.shape[:2]))
    F_none = o.residual(U, Uo, Uo1, dt, dt_old)
    assert np.abs(F_cpu - F_none).max() > 1e-6 * np.abs(F_cpu).max()         # the source is not lost in the rest
    f = forms.Expression(tof.SOURCE_STRING, D=tof.DE, w=tof.WEZ, alpha=tof.ALPHA_E, t=t0 + dt, pi=np.pi, degree=k)
    ops, consts, names = forms.expression_program(f)
    prob.set_ext_source_program(0, ops, consts, len(names))
    prob.set_state(U, Uo, Uo1)
    prob.set_step(dt, dt_old)
    for how in ("uploaded", "evaluated"):
        prob.set_ext_source(0, np.zeros(nodes.shape[:2]))
        if how == "uploaded":
            prob.set_ext_source(0, np.asarray(f(nodes)))
        else:
            prob.eval_ext_source(0, [getattr(f, n) for n in names])
            table, host = prob.get_ext_source(0), np.asarray(f(nodes))
            assert table.shape == host.shape and np.allclose(table, host, rtol=1e-11, atol=0.0)   # (exp of -100: ulps x 100)
        F_gpu, _ = prob.residual()
        assert np.abs(F_gpu - F_cpu).max() / np.abs(F_cpu).max() < 1e-11, how
        prob.jacobian()
        assert _rel_rows(prob.jacobian_csr(), J_cpu) < 1e-10, how
    prob.close()


# ---- two species ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degrees", [[0, 2], [2, 2]])
@pytest.mark.parametrize("name", ["structured", "delaunay"])
def test_two_species_keep_their_own_tables(name, degrees):
    from oracle import tof as otof
    from oracle.forms import LFAModel
    from oracle.mesh import Mesh as OMesh
    from fedm_amd.device import DeviceProblem
    m = _unit_meshes()[name]
    om = OMesh(m.coords, m.cells)
    prob = DeviceProblem(m.coords, m.cells, _model(degrees))
    o = LFAModel(om, 2, False, ["drift-diffusion-reaction"] * 2, [-1.0, -1.0], D=[0.12, 0.05],
                 drift_w=[(0.0, 1.7), (0.3, -0.5)], qdeg=8)
    nodes = otof.cell_nodes(om, 2)
    texts = {0: ("exp(-a*x[0])*x[1]", dict(a=0.8)), 1: ("3.0*sin(2.0*x[1])-x[0]", {})}
    tables = {}
    for s in (0, 1):
        if not degrees[s]:
            with pytest.raises(RuntimeError, match="no Expression source"):
                _run(prob, s, *texts[s][:1], **texts[s][1])
            with pytest.raises(RuntimeError, match="no Expression source"):
                prob.get_ext_source(s)
            continue
        tables[s], ops, consts, values = _run(prob, s, texts[s][0], **texts[s][1])
        want, tol = _tolerance(ops, consts, values, nodes)
        assert (np.abs(tables[s] - want) <= tol).all()
        o.set_ext_source(s, 2, want)
    for s in tables:                                   # the later program did not touch the earlier table
        assert np.array_equal(prob.get_ext_source(s), tables[s])
    if len(tables) == 2:
        assert np.abs(tables[0] - tables[1]).min() > 0
    rng = np.random.default_rng(2)
    U = rng.normal(0.0, 0.3, (om.nv, 2))
    Uo, Uo1 = U + rng.normal(0, 0.05, U.shape), U + rng.normal(0, 0.05, U.shape)
    dt, dt_old = 1e-2, 2e-2
    prob.set_state(U, Uo, Uo1)
    prob.set_step(dt, dt_old)
    F_gpu, _ = prob.residual()
    F_cpu, J_cpu = o.residual_jacobian(U, Uo, Uo1, dt, dt_old)
    for s in tables:                                   # each source is a visible part of its own rows
        o_none = o.ext_source[s]
        o.ext_source[s] = None
        F_none = o.residual(U, Uo, Uo1, dt, dt_old)
        o.ext_source[s] = o_none
        part = np.abs(F_cpu - F_none).reshape(-1, 2)
        assert part[:, s].max() > 1e-3 * np.abs(F_cpu).reshape(-1, 2)[:, s].max() and part[:, 1 - s].max() == 0
    scale = np.abs(F_cpu).reshape(-1, 2).max(axis=0)
    assert (np.abs(F_gpu - F_cpu).reshape(-1, 2) / scale).max() < 1e-11
    prob.jacobian()
    assert _rel_rows(prob.jacobian_csr(), J_cpu) < 1e-10
    prob.close()
