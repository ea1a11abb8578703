"""mimi_amd.solid.resolve_route without a GPU: every refusal of a flag combination, one row each, matched on the message
fragments the GPU tests use, and the Route a handful of accepted combinations resolve to.  A refused combination is refused
by setup() with the same text, before any device work."""
import pytest

from _explicit_cases import facade

ITERATIVE = ("use_iterative_solver",)
KRONECKER = ITERATIVE + ("use_kronecker_preconditioner",)
MATRIX_FREE = KRONECKER + ("matrix_free",)
BOUNDARY = MATRIX_FREE + ("matrix_free_boundary",)
EXPLICIT = ("explicit_dynamics",)
CONSISTENT = EXPLICIT + ("explicit_consistent_mass",)

# (flags set to 1, marker, periodic pair, MIMI_HIP_HOST_SETUP, fragment of the refusal)
REFUSED = [
    (("explicit_consistent_mass",), None, False, None, "needs explicit_dynamics"),
    (EXPLICIT + ("matrix_free",), None, False, None, "explicit_dynamics cannot be combined with matrix_free"),
    (EXPLICIT + ITERATIVE, None, False, None, "explicit_dynamics cannot be combined with use_iterative_solver"),
    (EXPLICIT + ("host_setup",), None, False, None, "explicit_dynamics cannot be combined with host_setup"),
    (EXPLICIT, None, False, "1", "explicit_dynamics cannot be combined with the host set-up"),
    (KRONECKER + ("matrix_free_boundary",), None, False, None, "matrix_free_boundary needs matrix_free"),
    (("matrix_free",), None, False, None, "matrix_free needs use_iterative_solver"),
    (ITERATIVE + ("matrix_free",), None, False, None, "use_kronecker_preconditioner"),
    (("use_kronecker_preconditioner", "matrix_free"), None, False, None, "matrix_free needs use_iterative_solver"),
    (MATRIX_FREE, "contact", False, None, "matrix_free cannot be combined with a contact marker"),
    (MATRIX_FREE, "pressure", False, None, "matrix_free cannot be combined with a follower pressure marker"),
    (KRONECKER, None, True, None, "periodic 1-D matrices"),
    (CONSISTENT, None, True, None, "explicit_consistent_mass cannot be combined with a periodic boundary"),
    # the first rule broken is the one reported: the Kronecker rule, the explicit rules, the consistent-mass rules, the
    # boundary-action rule, the matrix-free rules (solver flags, contact, pressure, pair), the host set-up by environment
    (MATRIX_FREE, None, True, None, "periodic 1-D matrices"),
    (BOUNDARY + EXPLICIT, "contact", True, None, "periodic 1-D matrices"),
    (EXPLICIT + ("matrix_free", "matrix_free_boundary", "host_setup"), None, False, None,
     "explicit_dynamics cannot be combined with matrix_free"),
    (EXPLICIT + ITERATIVE + ("host_setup", "explicit_consistent_mass"), None, True, None,
     "explicit_dynamics cannot be combined with use_iterative_solver"),
    (("explicit_consistent_mass", "matrix_free_boundary"), None, True, None, "needs explicit_dynamics"),
    (CONSISTENT + ("matrix_free_boundary",), None, True, None, "explicit_consistent_mass cannot be combined with a periodic boundary"),
    (ITERATIVE + ("matrix_free", "matrix_free_boundary"), "contact", False, None, "matrix_free needs use_iterative_solver"),
    (("matrix_free_boundary",), "contact", False, "1", "matrix_free_boundary needs matrix_free"),
]


def prepared(flags, marker, pair, host_env, monkeypatch):
    """(rc, bc, axes) of cube_p2 with the flags, a contact or pressure marker on the top, the pair (3, 5): no device work"""
    def configure(bc):
        from mimi_amd.integrators import RigidPlane
        for c in range(3):
            bc.initial.dirichlet(0, c)
        if marker == "contact":
            bc.current.contact(1, RigidPlane([0.0, 0.0, 2.0], [0.0, 0.0, -1.0]))
        if marker == "pressure":
            bc.initial.pressure(1, 3.0)
        if pair:
            bc.initial.periodic(3, 5)
    if host_env is None:
        monkeypatch.delenv("MIMI_HIP_HOST_SETUP", raising=False)
    else:
        monkeypatch.setenv("MIMI_HIP_HOST_SETUP", host_env)
    nl = facade("cube_p2", "neohook", flags=tuple((k, 1) for k in flags), configure=configure, setup=False)
    bc = nl.boundary_condition
    return nl, nl.runtime_communication, bc, nl._periodic_axes(bc)


@pytest.mark.parametrize("flags, marker, pair, host_env, fragment", REFUSED)
def test_refusals(flags, marker, pair, host_env, fragment, monkeypatch):
    import re
    from mimi_amd import solid
    nl, rc, bc, axes = prepared(flags, marker, pair, host_env, monkeypatch)
    assert axes == ([1] if pair else [])
    with pytest.raises(RuntimeError, match=re.escape(fragment)) as direct:
        solid.resolve_route(rc, bc, axes)
    with pytest.raises(RuntimeError, match=re.escape(fragment)) as through_setup:       # no device here: raised before any is needed
        nl.setup(1)
    assert str(direct.value) == str(through_setup.value)


# (flags, marker, pair, MIMI_HIP_HOST_SETUP, the fields of the Route that are set)
ACCEPTED = [
    ((), None, False, None, ()),
    ((), "contact", True, None, ()),
    (ITERATIVE, "pressure", True, None, ("iterative",)),
    (KRONECKER, "contact", False, None, ("iterative", "kronecker")),
    (("use_kronecker_preconditioner",), None, True, None, ()),                  # the preconditioner of the iterative solver only
    (KRONECKER + ("periodic_iterative",), None, True, None, ("iterative", "kronecker", "periodic_iterative")),
    (KRONECKER + ("periodic_iterative",), None, False, None, ("iterative", "kronecker")),       # no pair: nothing to switch
    (MATRIX_FREE, None, False, None, ("iterative", "kronecker", "matrix_free")),
    (BOUNDARY, "contact", False, None, ("iterative", "kronecker", "matrix_free", "boundary_actions")),
    (BOUNDARY + ("periodic_iterative",), "pressure", True, None,
     ("iterative", "kronecker", "matrix_free", "boundary_actions", "periodic_iterative")),
    (EXPLICIT, "contact", True, None, ("explicit",)),
    (CONSISTENT, None, False, None, ("explicit", "explicit_consistent")),
    (CONSISTENT + ("periodic_iterative",), None, True, None, ("explicit", "explicit_consistent", "periodic_iterative")),
    (("host_setup",), None, True, None, ("host_setup",)),
    (ITERATIVE, None, False, "1", ("iterative", "host_setup")),
    ((), None, False, "0", ()),
]


@pytest.mark.parametrize("flags, marker, pair, host_env, fields", ACCEPTED)
def test_accepted_routes(flags, marker, pair, host_env, fields, monkeypatch):
    from mimi_amd import solid
    nl, rc, bc, axes = prepared(flags, marker, pair, host_env, monkeypatch)
    route = solid.resolve_route(rc, bc, axes)
    assert route == solid.Route(**{k: True for k in fields})
    assert all(type(v) is bool for v in route)
    with pytest.raises(AttributeError):
        route.explicit = True


def test_no_runtime_communication_is_the_default_route(monkeypatch):
    from mimi_amd import solid
    nl, rc, bc, axes = prepared((), None, True, None, monkeypatch)
    assert solid.resolve_route(None, bc, axes) == solid.Route()
