"""The launches of the fused multigrid-preconditioned CG loop on a real MI355X (-m gpu):
tfem_pcg_start, then two steps of (tfem_cg_dot with the mask as inv_diag, tfem_pcg_update,
tfem_pcg_rz, tfem_pcg_direction) on synthetic data, every launch against numpy in long double.

Sizes: those of tests/test_hip_fused_cg.py's ``kernel_sizes`` (1, the wave edges 63 / 64 / 65, 257,
and one trip of the capped grid for THE instance plus 77 rows, so that every lane walks a second
time and the rows end in a ragged group), and 255, 256 (one workgroup and the row before it) and
1288 = 5 workgroups + 8 rows (a ragged last group below the cap).  n_vec = 1, 2, 4, 8 (the 16-byte
instances), 3 (the generic pass) and 9 (its second pass); float64 and float32; and every vector once
as a view that starts one element into its storage, where the widths 1, 2, 4, 8 take the generic
pass.

Data: ap = d * p and z = e * r with d, e > 0, so every term of every sum is positive and the
reductions have condition 1.  A fifth of the mask is exactly 0 (held rows; the free rows carry 1 or
0.5: only "zero or not" may matter) with ap = NaN and z = NaN there, one column is inactive, the
workspace and the start's p begin as NaN: a finite result proves that held rows are skipped and
that every partial sum a launch reads has been written.  Two steps, so both parities of r.z and
r.r are read and written.

Bounds: the ones tests/test_hip_fused_cg.py derives for the same arithmetic, U = 2^-53 (the sums are
accumulated in double for both types), u_T the unit roundoff of the vectors' type:
  a sum read back from the workspace is within ((n + 4) U + 2 u_T) of the long-double sum, relative;
  an updated entry a + s * b (x + alpha p, r - alpha ap, z + beta p) is within
  ((2 n + 8) U + 4 u_T) (|a| + |s b|) of the long-double value.
Every launch may change only what it is there to change: the other vectors and the other four
buffers of the workspace keep their bits, held rows and the inactive column of x, r and p keep
theirs (the column's r.r partials are still written), and two identical call sequences give
bit-identical vectors and workspace."""

import numpy as np
import pytest
import torch

from test_hip_fused_cg import LD, U, host, kernel_sizes, shifted, within

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 3, 4, 8, 9]
DTYPES = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["float64", "float32"])
#: the buffers of the workspace
PAP, RZ0, RR0, RZ1, RR1 = range(5)


@pytest.fixture(autouse=True)
def _gpu_defaults():
    assert torch.cuda.is_available()
    torch.set_default_dtype(torch.float64)
    torch.set_default_device("cuda")
    yield
    torch.set_default_device("cpu")
    torch.set_default_dtype(torch.float32)


def sizes_of(k, dtype):
    return tuple(sorted(set(kernel_sizes(k, dtype)) | {255, 256, 1288}))


def bits(t):
    """The tensor's bits as integers: NaN compares equal to the same NaN."""
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


class Launches:
    """The five launches of an iteration on torch tensors."""

    def __init__(self, n, k, dtype):
        from pytorch_fem_solver_amd import _native

        self.nat, self.lib = _native, _native.load()
        self.size = (torch.empty(0, dtype=dtype).element_size(), n, k)
        self.stream = _native.current_stream(torch.device("cuda"))

    def _go(self, fn, *args):
        self.nat.check(fn(*[self.nat.ptr(a) if torch.is_tensor(a) else a for a in args], self.stream))

    def start(self, r, z, mask, p, ws):
        self._go(self.lib.tfem_pcg_start, r, z, mask, p, *self.size, ws)

    def dot(self, p, ap, mask, ws):
        self._go(self.lib.tfem_cg_dot, p, ap, mask, *self.size, ws)

    def update(self, x, r, p, ap, mask, active, step, ws):
        self._go(self.lib.tfem_pcg_update, x, r, p, ap, mask, active, *self.size, step, ws)

    def rz(self, r, z, mask, step, ws):
        self._go(self.lib.tfem_pcg_rz, r, z, mask, *self.size, step, ws)

    def direction(self, p, z, mask, active, step, ws):
        self._go(self.lib.tfem_pcg_direction, p, z, mask, active, *self.size, step, ws)


def run_steps(n, k, dtype, seed, place=lambda t: t, check=True):
    """start, then two iterations (dot, update, rz, direction) on synthetic data.  `place` puts every
    vector where the launches find it (`shifted`: off the 16-byte alignment).  With `check` every
    launch is compared with numpy and with what it may not touch; without, the launches alone run
    (the second run of the bit-for-bit comparison).  Returns the final (x, r, p, ws)."""
    from pytorch_fem_solver_amd.sparse import cg_workspace

    npt = np.float64 if dtype == torch.float64 else np.float32
    u_t = float(np.finfo(npt).eps) / 2
    rng = np.random.default_rng(seed)
    held = rng.random(n) < 0.2
    held[0] = False  # at least one free row: the sums are positive
    mask_np = np.where(rng.random(n) < 0.5, 1.0, 0.5).astype(npt)
    mask_np[held] = 0
    free = ~held
    d = rng.uniform(0.5, 2.0, (n, 1)).astype(npt)
    e = rng.uniform(0.5, 2.0, (2, n, 1)).astype(npt)
    active_np = np.ones(k, dtype=np.int32)
    if k > 1:
        active_np[k // 2] = 0
    on = active_np != 0
    off_t = torch.tensor(~on)
    x = place(torch.tensor(rng.standard_normal((n, k)).astype(npt)))
    r = place(torch.tensor(rng.standard_normal((n, k)).astype(npt)))
    # the steps run on a direction of their own (with the start's p = z and ap = d * p a system of
    # one row would be solved by the first step: r = 0 and 0 / 0 in the second)
    p = place(torch.tensor(rng.standard_normal((n, k)).astype(npt)))
    p_start = place(torch.full((n, k), float("nan"), dtype=dtype))
    dev_d, dev_e, dev_held = torch.tensor(d), torch.tensor(e), torch.tensor(held)
    mask, active = place(torch.tensor(mask_np)), torch.tensor(active_np)
    ws = cg_workspace(n, k, x.device)
    assert ws.shape[0] == 5 and ws.shape[2] == k and ws.dtype == torch.float64
    ws.fill_(float("nan"))
    go = Launches(n, k, dtype)
    sum_tol = (n + 4) * U + 2 * u_t
    step_tol = LD((2 * n + 8) * U + 4 * u_t)

    def z_of(r, which):
        z = place(dev_e[which] * r)
        z[dev_held] = float("nan")
        return z

    def launch(what, fn, *args, writes=(), buffer=None):
        """Runs the launch; with `check`, every vector of `args` that is not in `writes` and every
        buffer of the workspace but `buffer` must keep its bits, and `buffer` must come out finite."""
        if not check:
            fn(*args)
            return
        vectors = [a for a in args if torch.is_tensor(a) and a is not ws and all(a is not w for w in writes)]
        before, ws_before = [bits(v).clone() for v in vectors], bits(ws).clone()
        fn(*args)
        for v, b in zip(vectors, before):
            assert torch.equal(bits(v), b), f"{what}: an input was written"
        for i in range(5):
            if i != buffer:
                assert torch.equal(bits(ws)[i], ws_before[i]), f"{what}: buffer {i} of the workspace was written"
        if buffer is not None:
            assert np.isfinite(host(ws[buffer])).all(), f"{what}: a partial of buffer {buffer} was not written (or a held row was read)"

    def check_sum(buffer, a_np, b_np, what):
        """The buffer's sum over the workgroups against sum a * b over the free rows, every column."""
        if not check:
            return None
        want = (a_np.astype(LD) * b_np.astype(LD))[free].sum(0)
        within(host(ws[buffer].sum(0)), want, sum_tol * want, what)
        return want

    # ---- start: p = z on the free rows (bit for bit), 0 on the held ones; r.z into parity 1
    z = z_of(r, 0)
    launch("start", go.start, r, z, mask, p_start, ws, writes=(p_start,), buffer=RZ1)
    if check:
        assert torch.equal(bits(p_start[~dev_held]), bits(z[~dev_held])), "start: p != z on a free row"
        assert bool((p_start[dev_held] == 0).all()), "start: p != 0 on a held row"
    rz_prev = check_sum(RZ1, host(r), host(z), "start: sum r.z")

    for step in (0, 1):
        what = f"n = {n}, k = {k}, {npt.__name__}, step {step}"
        par = step & 1
        ap = place(dev_d * p)
        ap[dev_held] = float("nan")
        x0, r0, p0 = x.clone(), r.clone(), p.clone()
        x0_np, r0_np, p0_np = host(x0).astype(LD), host(r0).astype(LD), host(p0).astype(LD)
        ap_np = host(ap).astype(LD)
        # ---- dot: the existing launch, the mask in the place of inv_diag
        launch(f"{what}: dot", go.dot, p, ap, mask, ws, buffer=PAP)
        pap = check_sum(PAP, host(p0), host(ap), f"{what}: sum p.Ap")
        # ---- update: reads p.Ap and r.z of the other parity, writes r.r of this one and no r.z
        launch(f"{what}: update", go.update, x, r, p, ap, mask, active, step, ws, writes=(x, r), buffer=RR1 if par else RR0)
        if check:
            alpha = np.where(on, rz_prev / pap, LD(0))
            moved = free[:, None] & on[None, :]
            step_ap = alpha * np.where(moved, ap_np, 0)
            want_x = np.where(moved, x0_np + alpha * p0_np, x0_np)
            want_r = np.where(moved, r0_np - step_ap, r0_np)
            within(host(x), want_x, step_tol * (np.abs(x0_np) + np.abs(alpha * p0_np)), f"{what}: x")
            within(host(r), want_r, step_tol * (np.abs(r0_np) + np.abs(step_ap)), f"{what}: r")
            assert torch.equal(x[dev_held], x0[dev_held]) and torch.equal(r[dev_held], r0[dev_held]), f"{what}: a held row moved"
            assert torch.equal(x[:, off_t], x0[:, off_t]) and torch.equal(r[:, off_t], r0[:, off_t]), f"{what}: the inactive column moved"
        # |r|^2 of every column, the inactive one included
        check_sum(RR1 if par else RR0, host(r), host(r), f"{what}: sum r.r")
        # ---- rz: the preconditioner has turned the new r into a new z
        z = z_of(r, 1)
        launch(f"{what}: rz", go.rz, r, z, mask, step, ws, buffer=RZ1 if par else RZ0)
        rz_new = check_sum(RZ1 if par else RZ0, host(r), host(z), f"{what}: sum r.z")
        # ---- direction: reads both r.z, writes no buffer
        launch(f"{what}: direction", go.direction, p, z, mask, active, step, ws, writes=(p,))
        if check:
            beta = np.where(on, rz_new / rz_prev, LD(0))
            z_np = np.where(free[:, None], host(z), 0).astype(LD)
            want_p = np.where(moved, z_np + beta * p0_np, p0_np)
            within(host(p), want_p, step_tol * (np.abs(z_np) + np.abs(beta * p0_np)), f"{what}: p")
            assert torch.equal(p[dev_held], p0[dev_held]), f"{what}: direction wrote a held row"
            assert torch.equal(p[:, off_t], p0[:, off_t]), f"{what}: direction wrote the inactive column"
        rz_prev = rz_new
    assert bool(torch.isfinite(ws).all())
    return x, r, p, ws


@DTYPES
@pytest.mark.parametrize("k", WIDTHS)
def test_pcg_launches_against_numpy(k, dtype):
    sizes = sizes_of(k, dtype)
    assert sizes[0] == 1 and {255, 256, 257, 1288} <= set(sizes) and sizes[-1] > 256 * 1024
    for n in sizes:
        first = run_steps(n, k, dtype, seed=1000 * k + n % 997)
        if n in (65, 1288, sizes[-1]):
            again = run_steps(n, k, dtype, seed=1000 * k + n % 997, check=False)
            for a, b, name in zip(first, again, ("x", "r", "p", "workspace")):
                assert torch.equal(a, b), f"n = {n}, k = {k}: {name} differs between two identical runs"


@DTYPES
@pytest.mark.parametrize("k", WIDTHS)
def test_pcg_launches_on_vectors_off_the_16_byte_alignment(k, dtype):
    """Every vector, the mask included, a view that starts one element into its storage: the widths
    with a 16-byte instance take the generic pass instead, each launch deciding from its own arrays.
    The same checks against numpy, to the same bounds."""
    for n in (1, 257, 1288):
        run_steps(n, k, dtype, seed=77 * k + n, place=shifted)
