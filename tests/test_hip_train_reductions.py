"""The train step's reduction kernels held to fp64 (tests/bn_oracle.py) at the edges of their grids: bn_stats / bn_apply / bn_finalize,
bn_bwd_reduce / bn_bwd_apply and psm_loss_sums / _grad, called the way engine.py, modeling/psmnet/train.py and utils/loss_utils.py do.

Geometry: bn_oracle.CASES a..n (one block ... 512 blocks, ragged and empty trailing blocks, every regime of blocked_walk.h's walk_rows,
the 2D layout, a channel-block slice); each case asserts through bn_oracle.launch_plan that it reaches the grid it is named for.
Input: bn_oracle.trend_input -- every row block has its own mean, and for every case with a ragged or empty block the test first shows,
in fp64 on the CPU, that merging the chunks with equal weights or dropping the last one moves mean and variance by >= 10x the tolerance.
Inputs live in NaN-filled storage (a kernel that reads a halo or a neighbouring channel block turns NaN), outputs in storage pre-filled
with a sentinel that must survive everywhere outside the interior.

Bounds (none of them fitted to what the kernels give):
  bn_stats        mean, variance  <= 1e-5 * max|ref| each (tests/test_hip_train.py's bound), padded channels exactly 0, M2 >= 0
  bn_apply        <= 2e-5 * max(1, max|ref|) with the kernel's own fp32 mean / invstd (the same test's bound)
  bn_bwd_reduce   |err| <= 1e-5 * sum|terms| per channel: <= ~100 sequential fp32 additions per value (a thread's run of rows, then the
                  64-deep fixed-order finish) is <= 6e-6 of sum|terms|; one dropped chunk of 512 voxels is >= 2e-3 of it.  The test
                  asserts |sum| >= 0.2 * sum|terms| on the reference, so the bound is relative to the sums themselves within 5x
  bn_bwd_apply    <= 2e-5 * max(1, max|ref|) against the oracle evaluated with the kernel's own sums
  conditioning    kappa = sqrt(1 + mean^2/var): variance relative error <= 2^-22 * kappa + 2^-20, mean error <= 2^-21 * max(|mu|, sigma)
                  (a shifted one-pass / Chan scheme is O(eps * kappa), eps = 2^-24; sum x^2 - n mean^2 is off by 1e-2 .. > 1 here)
  bn_finalize     1e-6 relative per value (three fp32 roundings and a 1-ulp rsqrt; the inputs are positive, so the running update
                  does not cancel), counter exact
  loss            sums 0, 1, 2, 4 within 1e-5 relative (non-negative terms), sums[3] exact; gradient <= 1e-6 * max|ref|, exact zeros

Every test prints its measured error next to the bound (run with -s).  The conditioning ratios (variance error in eps*kappa, mean
error in eps*|mu|) have not been recorded from an MI355X yet: the fp32 emulation of the merge order on the CPU gave <= 0.1 eps*kappa
and <= 1.7 eps*|mu|; test_bn_stats_conditioning prints the GPU's figures, which belong here.
"""
import pytest
import torch
from torch import nn

from oracle import psmnet_oracle as O
from disprcnn_amd.utils import synth
from tests import bn_oracle as B

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENT = 7.25
NAN = float("nan")
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ blocked tensors without the pack kernels
def _alloc(E, name, dev, fill):
    """A Blocked tensor of case `name` (case n: channel blocks [2, 5) of a 7-block tensor) whose WHOLE storage holds `fill`."""
    (N, C, D, H, W), halo, _ = B.CASES[name]
    if name == "n":
        base = E.Blocked(N, 7 * 16, D, H, W, *halo, dev)
        base.storage.fill_(fill)
        return E.BlockedSlice(base, 2, C)
    t = E.Blocked(N, C, D, H, W, *halo, dev)
    t.storage.fill_(fill)
    return t


def _interior_of(t, storage):
    base = getattr(t, "base", t)
    off = getattr(t, "cb_off", 0)
    v = storage[: base.numel].view(base.N, base.cb, base.Dp, base.Hp, base.Wp, 16)
    return v[:, off:off + t.cb, t.pd:t.pd + t.D, t.ph:t.ph + t.H, t.pw:t.pw + t.W]


def _put(t, dense):
    """dense [N,C,D,H,W] (CPU) -> the interior of t; the padded channels of the last block become 0."""
    N, C = dense.shape[:2]
    full = torch.zeros(N, t.cb * 16, *dense.shape[2:], dtype=torch.float32)
    full[:, :C] = dense
    _interior_of(t, t.storage).copy_(full.view(N, t.cb, 16, t.D, t.H, t.W).permute(0, 1, 3, 4, 5, 2).to(t.storage.device))
    return t


def _get(t, channels=None):
    """interior of t -> dense [N, cb*16 (or `channels`), D, H, W] on the CPU"""
    d = _interior_of(t, t.storage).permute(0, 1, 5, 2, 3, 4).reshape(t.N, t.cb * 16, t.D, t.H, t.W).cpu()
    return d if channels is None else d[:, :channels]


def _outside_keeps(t, fill):
    """True when everything but the interior of t -- halo, slack, and for a slice the other channel blocks -- still holds `fill`."""
    s = t.storage.clone()
    _interior_of(t, s).fill_(fill)
    return bool((s == fill).all())


def _pad16(v, cb, dev):
    out = torch.zeros(cb * 16, dtype=torch.float32)
    out[: v.numel()] = v
    return out.to(dev)


def _say(name, what, err, bar):
    print(f"[{name}] {what}: err {err:.3e}  bound {bar:.3e}  ({err / bar if bar > 0 else 0.0:.3f} of it)")


# ------------------------------------------------------------------------------------------------ one context per geometry case
class Ctx:
    def __init__(self, name, dev):
        from disprcnn_amd import engine as E
        from disprcnn_amd import _lib
        self.E, self.lib, self._lib, self.dev, self.name = E, _lib.lib(), _lib, dev, name
        self.shape, self.halo, self.want = B.CASES[name]
        N, C, D, H, W = self.shape
        self.C, self.M = C, N * D * H * W
        self.plan = B.launch_plan(N, D, H, W)
        self.x = B.trend_input(f"trend:{name}", self.shape)
        self.xb = _put(_alloc(E, name, dev, NAN), self.x)
        self.cb = self.xb.cb
        self.stats, M = E.bn_batch_stats_raw(self.xb)
        assert M == self.M
        self.bn = nn.BatchNorm3d(C).to(dev).train()
        self.invstd = E.bn_finalize(self.stats, self.M, self.bn, C)
        self.mean = self.stats[0]
        self.gamma = _pad16(synth.hash_uniform(f"{name}:g", (C,), 0.5, 1.5), self.cb, dev)
        self.beta = _pad16(synth.hash_uniform(f"{name}:b", (C,), -0.5, 0.5), self.cb, dev)
        self._memo = {}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def alloc(self, fill):
        return _alloc(self.E, self.name, self.dev, fill)

    @property
    def res(self):
        return self.memo("res", lambda: synth.hash_uniform(f"{self.name}:r", self.shape, -1.0, 1.0))

    @property
    def resb(self):
        return self.memo("resb", lambda: _put(self.alloc(NAN), self.res))

    @property
    def xhat(self):
        """fp64 xhat from the kernel's fp32 statistics"""
        m, i = self.mean[: self.C].cpu().to(F64).view(1, -1, 1, 1, 1), self.invstd[: self.C].cpu().to(F64).view(1, -1, 1, 1, 1)
        return self.memo("xhat", lambda: (self.x.to(F64) - m) * i)

    @property
    def dy(self):
        """0.5 + 0.25 xhat + 0.1 u: neither sum_dz nor sum_dz_xhat cancels"""
        return self.memo("dy", lambda: (0.5 + 0.25 * self.xhat + 0.1 * synth.hash_uniform(f"{self.name}:dy", self.shape).to(F64)).float())

    @property
    def dyb(self):
        return self.memo("dyb", lambda: _put(self.alloc(NAN), self.dy))

    @property
    def yb_relu(self):
        """the output of bn_apply with ReLU (no residual): the mask of the backward"""
        def make():
            y = self.alloc(SENT)
            self.E.bn_apply(self.xb, y, None, self.mean, self.invstd, self.gamma, self.beta, True)
            return y
        return self.memo("yb", make)

    def bwd_reduce(self, relu, scratch=None):
        E = self.E
        sums = torch.full((2, self.cb * 16), SENT, dtype=torch.float32, device=self.dev)
        scratch = E.bn_scratch(self.dev, self.cb) if scratch is None else scratch
        y = self.yb_relu
        st = self.lib.drc_bn_bwd_reduce(E._ptr(self.dyb.storage), E._geom8(self.dyb), E._ptr(y.storage), E._geom8(y), E._ptr(self.xb.storage),
                                        E._geom8(self.xb), E._ptr(self.mean), E._ptr(self.invstd), int(relu), E._ptr(sums), E._ptr(scratch),
                                        E._stream_ptr(self.dev))
        self._lib.check(st, "drc_bn_bwd_reduce")
        return sums


@pytest.fixture(scope="module", params=sorted(B.CASES))
def ctx(request, dev):
    c = Ctx(request.param, dev)
    yield c
    c._memo.clear()
    del c
    torch.cuda.empty_cache()


def test_bn_stats(ctx):
    E, name, C = ctx.E, ctx.name, ctx.C
    assert B.grid_of(ctx.plan) == (ctx.want["blocks"], ctx.want["empty"], ctx.want["last"])
    if "rpb" in ctx.want:
        assert ctx.plan["rpb"] == ctx.want["rpb"]
    ref_m, ref_v = B.stats(ctx.x)
    tol_m, tol_v = 1e-5 * float(ref_m.abs().max()), 1e-5 * float(ref_v.abs().max())
    if B.is_ragged(ctx.plan):          # is the input strong enough to see a wrong merge?  (fp64, CPU)
        for mname, (mm, mv) in B.stat_mutants(ctx.x, ctx.plan).items():
            dm, dv = float((mm - ref_m).abs().max()), float((mv - ref_v).abs().max())
            print(f"[{name}] mutant {mname}: mean off by {dm / tol_m:.0f}x tol, variance by {dv / tol_v:.0f}x tol")
            assert dm >= 10 * tol_m and dv >= 10 * tol_v, f"input too weak for mutant {mname}"
    stats = ctx.stats.cpu()
    mean, m2 = stats[0], stats[1]
    em, ev = float((mean[:C].to(F64) - ref_m).abs().max()), float((m2[:C].to(F64) / ctx.M - ref_v).abs().max())
    _say(name, "bn_stats mean", em, tol_m)
    _say(name, "bn_stats var ", ev, tol_v)
    assert em <= tol_m and ev <= tol_v
    assert (m2 >= 0).all()
    assert torch.equal(stats[:, C:], torch.zeros_like(stats[:, C:]))               # padded channels: exactly zero
    again, _ = E.bn_batch_stats_raw(ctx.xb)
    assert torch.equal(again.cpu(), stats)
    # the variance engine.bn_batch_stats reports is this M2 / M
    m_, v_, M_ = E.bn_batch_stats(ctx.xb)
    assert M_ == ctx.M and torch.equal(m_.cpu(), mean) and (v_.cpu() - m2 / ctx.M).abs().max() <= 1e-6 * (m2 / ctx.M).max()


def test_bn_apply(ctx):
    E, name, C = ctx.E, ctx.name, ctx.C
    mean, invstd = ctx.mean[:C].cpu(), ctx.invstd[:C].cpu()
    for with_res in (False, True):
        for relu in (False, True):
            y = ctx.alloc(SENT)
            E.bn_apply(ctx.xb, y, ctx.resb if with_res else None, ctx.mean, ctx.invstd, ctx.gamma, ctx.beta, relu)
            ref = B.apply(ctx.x, mean, invstd, ctx.gamma[:C].cpu(), ctx.beta[:C].cpu(), ctx.res if with_res else None, relu)
            got = _get(y)
            err, bar = float((got[:, :C].to(F64) - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
            _say(name, f"bn_apply res={int(with_res)} relu={int(relu)}", err, bar)
            assert err <= bar
            assert torch.isfinite(got).all() and _outside_keeps(y, SENT)
            if relu:
                assert (got >= 0).all()


def test_bn_bwd_reduce(ctx):
    name, C = ctx.name, ctx.C
    y = _get(ctx.yb_relu, C)
    for relu in (False, True):
        ref = B.bwd(ctx.dy, y, ctx.x, ctx.mean[:C].cpu(), ctx.invstd[:C].cpu(), ctx.gamma[:C].cpu(), relu)
        for k, a in (("sum_dz", "sum_abs_dz"), ("sum_dz_xhat", "sum_abs_dz_xhat")):                  # the sums must not cancel
            assert (ref[k].abs() >= 0.2 * ref[a]).all(), f"{k} cancels: {float((ref[k].abs() / ref[a]).min()):.3f}"
        sums = ctx.bwd_reduce(relu).cpu()
        for row, (k, a) in enumerate((("sum_dz", "sum_abs_dz"), ("sum_dz_xhat", "sum_abs_dz_xhat"))):
            ratio = float(((sums[row, :C].to(F64) - ref[k]).abs() / ref[a]).max())
            _say(name, f"bn_bwd_reduce relu={int(relu)} {k} (per sum|terms|)", ratio, 1e-5)
            assert ratio <= 1e-5
        assert torch.equal(sums[:, C:], torch.zeros_like(sums[:, C:]))
        assert torch.equal(ctx.bwd_reduce(relu).cpu(), sums)


def test_bn_bwd_apply(ctx):
    E, name, C = ctx.E, ctx.name, ctx.C
    y = _get(ctx.yb_relu, C)
    prefill = synth.hash_uniform(f"{name}:dres0", ctx.shape, -1.0, 1.0)
    for relu, dres_mode in ((False, None), (True, "overwrite"), (False, "accumulate"), (True, "accumulate")):
        sums = ctx.bwd_reduce(relu)
        ref = B.bwd(ctx.dy, y, ctx.x, ctx.mean[:C].cpu(), ctx.invstd[:C].cpu(), ctx.gamma[:C].cpu(), relu, sums=sums[:, :C].cpu())
        draw = ctx.alloc(SENT)
        dres = None
        if dres_mode is not None:
            dres = ctx.alloc(SENT)
            if dres_mode == "accumulate":
                _put(dres, prefill)
        yb = ctx.yb_relu
        st = ctx.lib.drc_bn_bwd_apply(E._ptr(ctx.dyb.storage), E._geom8(ctx.dyb), E._ptr(yb.storage), E._geom8(yb), E._ptr(ctx.xb.storage),
                                      E._geom8(ctx.xb), E._ptr(ctx.mean), E._ptr(ctx.invstd), E._ptr(ctx.gamma), E._ptr(sums), 1.0 / ctx.M,
                                      int(relu), E._ptr(draw.storage), E._geom8(draw), E._ptr(dres.storage) if dres is not None else None,
                                      E._geom8(dres) if dres is not None else None, int(dres_mode == "accumulate"), E._stream_ptr(ctx.dev))
        ctx._lib.check(st, "drc_bn_bwd_apply")
        got = _get(draw)
        err, bar = float((got[:, :C].to(F64) - ref["draw"]).abs().max()), 2e-5 * max(1.0, float(ref["draw"].abs().max()))
        _say(name, f"bn_bwd_apply relu={int(relu)} draw", err, bar)
        assert err <= bar and torch.isfinite(got).all() and _outside_keeps(draw, SENT)
        if dres is not None:
            want = ref["dres"] + (prefill.to(F64) if dres_mode == "accumulate" else 0.0)
            got = _get(dres)
            err, bar = float((got[:, :C].to(F64) - want).abs().max()), 2e-5 * max(1.0, float(want.abs().max()))
            _say(name, f"bn_bwd_apply relu={int(relu)} dres {dres_mode}", err, bar)
            assert err <= bar and torch.isfinite(got).all() and _outside_keeps(dres, SENT)


def test_empty_batch_returns_without_touching_outputs(dev):
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    lib, sp = _lib.lib(), E._stream_ptr(dev)
    t = [E.Blocked(0, 16, 2, 3, 4, 1, 1, 1, dev) for _ in range(5)]
    for b in t:
        b.storage.fill_(SENT)
    x, y, dy, draw, dres = t
    vec = [torch.full((2, 16), SENT, device=dev) for _ in range(2)]
    stats, sums = vec
    par = torch.ones(16, device=dev)
    scratch = E.bn_scratch(dev, 1)
    g = E._geom8
    assert lib.drc_bn_stats_blocked(E._ptr(x.storage), g(x), E._ptr(stats), E._ptr(scratch), sp) == 0
    assert lib.drc_bn_apply_blocked(E._ptr(x.storage), g(x), E._ptr(y.storage), g(y), None, None, E._ptr(par), E._ptr(par), E._ptr(par),
                                    E._ptr(par), 1, sp) == 0
    assert lib.drc_bn_bwd_reduce(E._ptr(dy.storage), g(dy), E._ptr(y.storage), g(y), E._ptr(x.storage), g(x), E._ptr(par), E._ptr(par), 1,
                                 E._ptr(sums), E._ptr(scratch), sp) == 0
    assert lib.drc_bn_bwd_apply(E._ptr(dy.storage), g(dy), E._ptr(y.storage), g(y), E._ptr(x.storage), g(x), E._ptr(par), E._ptr(par),
                                E._ptr(par), E._ptr(sums), 1.0, 1, E._ptr(draw.storage), g(draw), E._ptr(dres.storage), g(dres), 1, sp) == 0
    torch.cuda.synchronize()
    for b in t:
        assert bool((b.storage == SENT).all())
    assert bool((stats == SENT).all()) and bool((sums == SENT).all())
    assert int(scratch[E.BN_MAX_CHUNKS * 32:].view(torch.int32).count_nonzero()) == 0
    # and through the engine's wrappers
    s, M = E.bn_batch_stats_raw(x)
    assert M == 0 and s.shape == (2, 16)
    E.bn_apply(x, y, None, par, par, par, par, True)


# ------------------------------------------------------------------------------------------------ ticket words
def test_ticket_words_rearm_between_grids(dev):
    """One stream, CB = 2, the shared scratch: 512 blocks, 1, 17 (one empty), 512 (64 empty), 16 -- bn_stats and bn_bwd_reduce
    alternating, then the same geometries with the two kernels swapped.  The ticket words are zero after every launch, stale partials
    (poisoned with NaN) are never read, and every result is the one a freshly zeroed scratch gives."""
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    lib, sp = _lib.lib(), E._stream_ptr(dev)
    CBN = 2
    shared = E.bn_scratch(dev, CBN)
    npart = E.BN_MAX_CHUNKS * CBN * 32
    assert shared.numel() == npart + CBN * 32 * 33
    gen = torch.Generator(device=dev).manual_seed(7)
    par_m = torch.rand(32, device=dev, generator=gen)
    par_i = torch.rand(32, device=dev, generator=gen) + 0.5
    tensors = {}
    for name in "jadkc":
        (N, _, D, H, W), halo, want = B.CASES[name]
        assert B.launch_plan(N, D, H, W)["blocks"] == want["blocks"]
        pair = []
        for _ in range(2):
            t = E.Blocked(N, 32, D, H, W, *halo, dev)
            t.storage.copy_(torch.rand(t.storage.numel(), device=dev, generator=gen))
            pair.append(t)
        tensors[name] = pair

    def launch(name, op, scratch):
        x, dy = tensors[name]
        out = torch.full((2, 32), SENT, device=dev)
        if op == "stats":
            st = lib.drc_bn_stats_blocked(E._ptr(x.storage), E._geom8(x), E._ptr(out), E._ptr(scratch), sp)
        else:
            st = lib.drc_bn_bwd_reduce(E._ptr(dy.storage), E._geom8(dy), E._ptr(x.storage), E._geom8(x), E._ptr(x.storage), E._geom8(x),
                                       E._ptr(par_m), E._ptr(par_i), 0, E._ptr(out), E._ptr(scratch), sp)
        _lib.check(st, op)
        return out

    for first in ("stats", "bwd"):
        ops = [first, "bwd" if first == "stats" else "stats"]
        for i, name in enumerate("jadkc"):
            op = ops[i % 2]
            shared[:npart].fill_(NAN)
            got = launch(name, op, shared)
            tickets = shared[npart:].view(torch.int32)
            assert int(tickets.count_nonzero()) == 0, f"ticket words left non-zero after {op} of case {name}"
            fresh = torch.zeros_like(shared)
            want = launch(name, op, fresh)
            assert int(fresh[npart:].view(torch.int32).count_nonzero()) == 0
            assert torch.isfinite(got).all() and torch.equal(got, want), f"{op} of case {name} differs from a fresh scratch"
            print(f"[ticket] {op:5s} case {name}: re-armed, equal to a fresh scratch")


# ------------------------------------------------------------------------------------------------ conditioning of the statistics
@pytest.mark.parametrize("mu,sigma", [(100.0, 0.1), (1000.0, 0.01), (-300.0, 0.05), (1000.0, 1.0)])
@pytest.mark.parametrize("name", ["c", "k"])
def test_bn_stats_conditioning(dev, name, mu, sigma):
    from disprcnn_amd import engine as E
    shape = B.CASES[name][0]
    C = shape[1]
    x = B.trend_input(f"cond:{name}:{mu}:{sigma}", shape, trend=False, mu=mu, sigma=sigma)
    xb = _put(_alloc(E, name, dev, NAN), x)
    stats, M = E.bn_batch_stats_raw(xb)
    stats = stats.cpu().to(F64)
    ref_m, ref_v = B.stats(x)                               # fp64 statistics of the fp32 data
    kappa = torch.sqrt(1.0 + ref_m ** 2 / ref_v)
    rel_v = (stats[1, :C] / M - ref_v).abs() / ref_v
    err_m = (stats[0, :C] - ref_m).abs()
    eps = 2.0 ** -24
    print(f"[cond {name} mu={mu} sigma={sigma}] kappa {float(kappa.max()):.3g}: variance rel err {float(rel_v.max()):.3e} = "
          f"{float((rel_v / (eps * kappa)).max()):.4f} eps*kappa ({float((rel_v / (2.0 ** -22 * kappa + 2.0 ** -20)).max()):.4f} of the bound); "
          f"mean err {float(err_m.max()):.3e} = {float(err_m.max()) / (eps * abs(mu)):.3f} eps*|mu| "
          f"({float(err_m.max()) / (2.0 ** -21 * max(abs(mu), sigma)):.4f} of the bound)")
    assert (rel_v <= 2.0 ** -22 * kappa + 2.0 ** -20).all()
    assert (err_m <= 2.0 ** -21 * max(abs(mu), sigma)).all()
    assert (stats[1] >= 0).all()


@pytest.mark.parametrize("name", ["c", "e", "k"])
def test_bn_stats_constant_input(dev, name):
    from disprcnn_amd import engine as E
    shape = B.CASES[name][0]
    C = shape[1]
    xb = _put(_alloc(E, name, dev, NAN), torch.full(shape, 3.7))
    stats, M = E.bn_batch_stats_raw(xb)
    bn = nn.BatchNorm3d(C).to(dev).train()
    invstd = E.bn_finalize(stats, M, bn, C).cpu().to(F64)
    mean, m2 = stats[0, :C].cpu().to(F64), stats[1, :C].cpu().to(F64)
    v37 = float(torch.tensor(3.7, dtype=torch.float32))
    print(f"[const {name}] mean err {float((mean - v37).abs().max()):.3e}  max M2 {float(m2.max()):.3e}  "
          f"invstd rel err {float((invstd * EPS ** 0.5 - 1).abs().max()):.3e}")
    assert (mean - v37).abs().max() <= 2.0 ** -23 * 3.7
    assert (m2 >= 0).all() and torch.isfinite(invstd).all()
    assert (invstd * EPS ** 0.5 - 1).abs().max() <= 1e-6


# ------------------------------------------------------------------------------------------------ bn_finalize
@pytest.mark.parametrize("M", [2, 1485, 301056])
@pytest.mark.parametrize("track", [True, False])
def test_bn_finalize(dev, M, track):
    from disprcnn_amd import engine as E
    C16, C = 48, 40
    mean = synth.hash_uniform("fin:m", (C16,), 0.5, 3.0)
    var = synth.hash_uniform("fin:v", (C16,), 0.2, 2.0)
    mean[C:] = 0; var[C:] = 0
    bn = nn.BatchNorm3d(C16, eps=EPS, momentum=0.1, track_running_stats=track).to(dev).train()
    rm = rv = None
    if track:
        rm, rv = synth.hash_uniform("fin:rm", (C16,), 0.5, 2.0), synth.hash_uniform("fin:rv", (C16,), 0.5, 2.0)
        with torch.no_grad():
            bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    for call in (1, 2):
        stats = torch.stack([mean * call, var * M / call]).to(dev)           # another batch on the second call
        versions = [t._version for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)] if track else None
        invstd = E.bn_finalize(stats, M, bn, C)
        ref_i, rm, rv = B.finalize(stats[0].cpu(), stats[1].cpu(), M, EPS, 0.1, rm, rv)
        e = float(((invstd[:C].cpu().to(F64) - ref_i[:C]).abs() / ref_i[:C]).max())
        assert invstd.shape == (C16,) and e <= 1e-6
        msg = f"[finalize M={M} track={track} call {call}] invstd rel err {e:.3e}"
        if track:
            e_m = float(((bn.running_mean[:C].cpu().to(F64) - rm[:C]).abs() / rm[:C].abs()).max())
            e_v = float(((bn.running_var[:C].cpu().to(F64) - rv[:C]).abs() / rv[:C].abs()).max())
            msg += f"  running_mean {e_m:.3e}  running_var {e_v:.3e}"
            assert e_m <= 1e-6 and e_v <= 1e-6
            assert int(bn.num_batches_tracked) == call
            # beyond C the buffers are not touched (the reference values carry on unchanged there)
            init_m, init_v = synth.hash_uniform("fin:rm", (C16,), 0.5, 2.0), synth.hash_uniform("fin:rv", (C16,), 0.5, 2.0)
            assert torch.equal(bn.running_mean[C:].cpu(), init_m[C:]) and torch.equal(bn.running_var[C:].cpu(), init_v[C:])
            rm[C:], rv[C:] = init_m[C:].to(F64), init_v[C:].to(F64)
            now = [t._version for t in (bn.running_mean, bn.running_var, bn.num_batches_tracked)]
            assert all(b > a for a, b in zip(versions, now))
        else:
            assert bn.running_mean is None and bn.num_batches_tracked is None
        print(msg)


# ------------------------------------------------------------------------------------------------ loss
GRID_CAP = 1024 * 256          # train_ops.hip grid_for: at most 1024 blocks of 256 threads, a grid-stride loop behind them
NUMELS = [1, 255, 256, 257, GRID_CAP - 1, GRID_CAP, GRID_CAP + 1, 3 * GRID_CAP + 77]


def _knee():
    one = torch.tensor(1.0, dtype=torch.float32)
    return torch.stack([one, -one, torch.nextafter(one, one * 0), -torch.nextafter(one, one * 0), torch.nextafter(one, one * 2),
                        -torch.nextafter(one, one * 2), one * 0])


def _loss_inputs(n):
    """tgt in [0, 48), three heads within +-2.5 of it; the LAST min(7, n) elements have tgt = 0 and pred = exactly +-1, the floats on
    both sides of +-1, and 0 (pred - tgt is then exact), rotated by one from head to head.  The last element of the first head is exactly 1."""
    tgt = synth.hash_uniform("loss:t", (n,), 0.0, 48.0)
    preds = [tgt + synth.hash_uniform(f"loss:p{k}", (n,), -2.5, 2.5) for k in range(3)]
    sp = _knee()
    for j in range(min(7, n)):
        tgt[n - 1 - j] = 0.0
        for k in range(3):
            preds[k][n - 1 - j] = sp[(j + k) % 7]
    return preds, tgt


def _masks(n):
    last = torch.zeros(n, dtype=torch.uint8)
    last[-1] = 1
    return {"ones": torch.ones(n, dtype=torch.uint8), "zero": torch.zeros(n, dtype=torch.uint8), "last": last,
            "rand60": (synth.hash_uniform("loss:m", (n,), 0.0, 1.0) < 0.6).to(torch.uint8)}


@pytest.mark.parametrize("form", ["train", "eval"])
@pytest.mark.parametrize("n", NUMELS)
def test_psm_loss_sums_and_grad(dev, n, form):
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    lib, sp = _lib.lib(), E._stream_ptr(dev)
    preds, tgt = _loss_inputs(n)
    d0 = preds[0][-min(7, n):] - tgt[-min(7, n):]
    assert n < 7 or {float(v) for v in d0} == {float(v) for v in _knee()}             # the knee values arrive exactly
    heads = preds if form == "train" else [preds[0], None, None]
    dp, dt = [p.to(dev) if p is not None else None for p in heads], tgt.to(dev)
    scratch = E.scratch(dev, "loss", _lib.LOSS_SCRATCH_FLOATS)
    gscale = torch.tensor([0.37], device=dev)

    def run_sums(dm):
        sums = torch.full((5,), SENT, device=dev)
        st = lib.drc_psm_loss_sums(E._ptr(dp[0]), E._ptr(dp[1]), E._ptr(dp[2]), E._ptr(dt), E._ptr(dm), n, E._ptr(sums), E._ptr(scratch), sp)
        _lib.check(st, "drc_psm_loss_sums")
        return sums

    for mname, mask in _masks(n).items():
        dm = mask.to(dev)
        sums = run_sums(dm)
        ref = B.loss_sums(heads[0], heads[1], heads[2], tgt, mask)
        got = sums.cpu().to(F64)
        assert float(got[3]) == float(mask.sum()) == float(ref[3])
        worst = 0.0
        for k in (0, 1, 2, 4):
            if ref[k] == 0:
                assert got[k] == 0, f"sums[{k}] of mask {mname}"
            else:
                worst = max(worst, float((got[k] - ref[k]).abs() / ref[k]))
        _say(f"loss n={n} {form} {mname}", "sums rel", worst, 1e-5)
        assert worst <= 1e-5
        assert torch.equal(run_sums(dm), sums)
        for k, w in enumerate((0.5, 0.7, 1.0)):
            if heads[k] is None:
                continue
            gp = torch.full((n,), SENT, device=dev)
            st = lib.drc_psm_loss_grad(E._ptr(dp[k]), E._ptr(dt), E._ptr(dm), n, E._ptr(sums), w, E._ptr(gscale), E._ptr(gp), sp)
            _lib.check(st, "drc_psm_loss_grad")
            gref = B.loss_grad(heads[k], tgt, mask, w, float(gscale.cpu()[0].to(F64)))
            g = gp.cpu()
            assert torch.isfinite(g).all()                                               # an empty mask divides by nothing
            assert torch.equal(g[mask == 0], torch.zeros_like(g[mask == 0]))
            err, bar = float((g.to(F64) - gref).abs().max()), 1e-6 * float(gref.abs().max())
            assert err <= bar, f"grad head {k} mask {mname}: {err:.3e} > {bar:.3e}"
            if mname == "zero":
                assert not g.any()


def test_psm_loss_sums_of_nothing(dev):
    from disprcnn_amd import engine as E
    from disprcnn_amd import _lib
    sums = torch.full((5,), SENT, device=dev)
    e = torch.empty(0, device=dev)
    st = _lib.lib().drc_psm_loss_sums(E._ptr(e), None, None, E._ptr(e), E._ptr(e), 0, E._ptr(sums), None, E._stream_ptr(dev))
    assert st == 0 and not sums.cpu().any()


@pytest.mark.parametrize("mname", ["ones", "zero", "last", "rand60"])
def test_loss_modules_vs_oracle(dev, mname):
    """PSMLoss / EndPointErrorLoss on a [2, 131, 97] map; with an empty mask the train loss is the undivided (zero) sum and the eval
    loss is 0, as the reference's utils/loss_utils.py:22-31."""
    from disprcnn_amd.utils.loss_utils import PSMLoss, EndPointErrorLoss
    shape = (2, 131, 97)
    n = 2 * 131 * 97
    preds, tgt = _loss_inputs(n)
    mask = _masks(n)[mname].view(shape)
    tgt = tgt.view(shape)
    preds = [p.view(shape) for p in preds]
    dp = [p.to(dev).requires_grad_() for p in preds]
    y = {"disparity": tgt.to(dev), "mask": mask.to(dev).bool()}
    loss = PSMLoss()(dp, y)
    (loss * 0.37).backward()
    p64 = [p.to(F64).requires_grad_() for p in preds]
    ref = O.psm_loss(p64, tgt.to(F64), mask.bool())
    (ref * 0.37).backward()
    ev = PSMLoss()(dp[0].detach(), y)
    epe = EndPointErrorLoss()(y["disparity"], dp[0].detach(), y["mask"])
    ref_ev = O.psm_loss(preds[0].to(F64), tgt.to(F64), mask.bool())
    if mname == "zero":
        assert float(loss) == 0 and float(ev) == 0 and float(epe) == 0 and float(ref) == 0 and float(ref_ev) == 0
        assert all(not p.grad.any() for p in dp)
        return
    e_t, e_e = abs(float(loss) - float(ref)) / float(ref), abs(float(ev) - float(ref_ev)) / float(ref_ev)
    print(f"[modules {mname}] train loss rel err {e_t:.3e}  eval {e_e:.3e}")
    assert e_t <= 1e-5 and e_e <= 1e-5 and float(epe) == float(ev)
    for p, q in zip(dp, p64):
        assert (p.grad.cpu().to(F64) - q.grad).abs().max() <= 1e-6 * q.grad.abs().max()
        assert not p.grad.cpu()[mask == 0].any()
    if mname == "ones":                                     # no mask = every pixel counts
        assert float(EndPointErrorLoss()(y["disparity"], dp[0].detach())) == float(ev)
