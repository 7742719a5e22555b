"""The sequence of tfem_mg_* calls of one V-cycle on a real MI355X, for a single vector, a block and
the P2 level: which entry points, in which order, on which level and with which ``first`` flag.
The calls are recorded by a proxy around the loaded library; nothing here holds a tolerance."""

import pytest
import torch

pytestmark = pytest.mark.gpu

S, R, P = "tfem_mg_smooth", "tfem_mg_restrict_residual", "tfem_mg_prolong_add"
#: position of (the size, ``first``, ``n_vec``) among the arguments of the smoothers
SMOOTH_ARGS = {S: (5, 6, None), S + "_multi": (5, 7, 6)}
#: position of ``n_vec`` among the arguments of the block transfers
N_VEC_ARG = {R + "_multi": 10, P + "_multi": 7}


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def stiffness(b):
    return b.v_grad @ b.v_grad.mT


class Recorder:
    """The loaded library with every call of a tfem_mg_* entry point noted in ``calls``."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tfem_mg_"):
            return fn

        def recorded(*args):
            self.calls.append((name, args))
            return fn(*args)

        return recorded


@pytest.fixture
def recorder(monkeypatch):
    from pytorch_fem_solver_amd import _native

    proxy = Recorder(_native.load())
    monkeypatch.setattr(_native, "load", lambda: proxy)
    return proxy


def seq(levels, nu, suffix=""):
    """The names of one cycle from level ``levels`` down and up again."""
    if levels == 0:
        return []
    return nu * [S + suffix] + [R + suffix] + seq(levels - 1, nu, suffix) + [P + suffix] + nu * [S + suffix]


def _hierarchy(kind, levels, nu):
    import pytorch_fem_solver_amd as tf

    return getattr(tf, kind)(tf.meshgen.unit_square(4, 0.25, 1), levels, stiffness, nu=nu, dtype=torch.float64,
                             dirichlet=True)


def _cycle_calls(recorder, cycle, r):
    del recorder.calls[:]
    cycle(r)
    return list(recorder.calls)


def _check_smooths(calls, mg, nu):
    """``first`` is 1 on the first sweep of each visit of a level and 0 on all others; the sizes
    follow the levels down and up."""
    sizes = [lv.n for lv in mg.levels]
    top = len(sizes) - 1
    want_sizes, want_first = [], []
    for l in range(top, 0, -1):  # down: nu sweeps, the first one starts from zero
        want_sizes += nu * [sizes[l]]
        want_first += [1] + (nu - 1) * [0]
    for l in range(1, top + 1):  # up: nu sweeps on what the way down left
        want_sizes += nu * [sizes[l]]
        want_first += nu * [0]
    smooths = [(name, args) for name, args in calls if name in SMOOTH_ARGS]
    assert [args[SMOOTH_ARGS[name][0]] for name, args in smooths] == want_sizes
    assert [args[SMOOTH_ARGS[name][1]] for name, args in smooths] == want_first


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("levels", [0, 2])
def test_single_cycle(recorder, levels, nu):
    mg = _hierarchy("GeometricMultigrid", levels, nu)
    calls = _cycle_calls(recorder, mg.vcycle, torch.randn(mg.levels[-1].n))
    assert [name for name, _ in calls] == seq(levels, nu)
    _check_smooths(calls, mg, nu)


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("levels", [0, 2])
def test_block_cycle(recorder, levels, nu):
    """The launches of the single cycle in their block forms, as many for k = 3 as for k = 1."""
    mg = _hierarchy("GeometricMultigrid", levels, nu)
    lengths = []
    for k in (1, 3):
        calls = _cycle_calls(recorder, mg.vcycle_multi, torch.randn(mg.levels[-1].n, k))
        assert [name for name, _ in calls] == seq(levels, nu, "_multi")
        for name, args in calls:
            n_vec = args[SMOOTH_ARGS[name][2]] if name in SMOOTH_ARGS else args[N_VEC_ARG[name]]
            assert n_vec == k, (name, n_vec, k)
        _check_smooths(calls, mg, nu)
        lengths.append(len(calls))
    assert lengths[0] == lengths[1]


@pytest.mark.parametrize("nu", [1, 2])
@pytest.mark.parametrize("levels", [0, 2])
def test_p2_cycle(recorder, levels, nu):
    """The P2 level's sweeps are the single smoother's, its transfers are its own, and between them
    lies the whole cycle of the P1 hierarchy."""
    mg = _hierarchy("P2Multigrid", levels, nu)
    calls = _cycle_calls(recorder, mg.vcycle, torch.randn(mg.levels[-1].n))
    assert [name for name, _ in calls] == (nu * [S] + ["tfem_mg_p2_restrict_residual"] + seq(levels, nu)
                                           + ["tfem_mg_p2_prolong_add"] + nu * [S])
    _check_smooths(calls, mg, nu)
