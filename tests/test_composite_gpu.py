"""Colour compositing on the device: mp_composite, mp_tr_composite_bwd and mp_tr_composite_bwd_det through the C ABI against the
float64 reference tests/composite_reference.py (a sort-based restatement and its torch autograd); the bounds are
tests/tolerances_composite.py, the measured maxima profiles/composite_colour.txt.

The cases are composite_reference.CASES: the siblings' shapes in their opaque regimes and, new, in thin regimes where the
background shows through the hit rays, so that the last-sample rule, T_bg bg, the T_bg adjoint with its exception for the very
last sample and d bg_rgb are compared at visible magnitudes.  Measures: forward outputs, d rgb and d bg_rgb per element,
absolute (the adjoints over the case's max |d rgb_values|); d sdf as max |error| over the case's max |d sdf| and, on the thin
cases, again over the last sample of every person on every ray plus all samples of the rays with bg_T >= 0.05, scaled by that
subset's maximum; d beta relative (to |d beta| where it is at least a tenth of the sum of the rays' absolute parts, which the CPU
test asserts for every committed case; to that sum otherwise)."""
import numpy as np
import pytest
import torch

from tests import composite_reference as CR
from tests import geometry_reference as G
from tests import tolerances_composite as TOL

pytestmark = pytest.mark.gpu

FWD = ("rgb_values", "fg_rgb_values", "normal_values", "acc", "acc_person", "bg_T")
GUARD_ROWS, TAIL = 2, 37          # table rows no ray refers to; floats past the last row of d sdf[p] / d rgb[p]
POISON = 777.0
MEASURED = {}                     # running maxima, printed by every test that measures


def _note(name, value):
    MEASURED[name] = max(MEASURED.get(name, 0.0), float(value))


def _report():
    print("[composite] measured maxima so far:", {k: f"{v:.3e}" for k, v in sorted(MEASURED.items())})


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _tables(c, keys):
    """device pointer tables of the case's per-person arrays, every array with GUARD_ROWS more rows (copies of the last row)
    -> (tables, the tensors to keep alive)"""
    from multiply_amd import hip
    pad = lambda a: np.concatenate([a, np.repeat(a[-1:], GUARD_ROWS, 0)], 0)
    keep = [[_dev(a if k == "inv" else pad(a)) for a in c[k]] for k in keys]
    return [hip.device_ints([t.data_ptr() for t in ts], "cuda") for ts in keep], keep


def _call(fn, args, raises):
    if raises is None:
        assert fn(*args) == 0
    else:
        with pytest.raises(RuntimeError, match=f"{fn.__name__} failed with code {raises}$"):
            fn(*args)
    torch.cuda.synchronize()


def forward(c, n_rays=None, white=False, guard=0, raises=None):
    """mp_composite on a case's numpy inputs -> {name: numpy output with `guard` poisoned rows past R}"""
    from multiply_amd import hip
    R, P, NZ = c["shape"]
    tabs, keep = _tables(c, ("inv", "z", "sdf", "rgb", "nrm"))
    beta_d = torch.tensor([c["beta"]], dtype=torch.float32, device="cuda")
    bg = None if white else _dev(c["bg"])
    cols = dict(rgb_values=(3,), fg_rgb_values=(3,), normal_values=(3,), acc=(), acc_person=(P,), bg_T=())
    bufs = {k: torch.full((R + guard,) + cols[k], POISON, dtype=torch.float32, device="cuda") for k in FWD}
    _call(hip.lib().mp_composite, (R if n_rays is None else n_rays, P, NZ, *tabs, beta_d, bg, *[bufs[k] for k in FWD], hip.stream()),
          raises)
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def backward(c, up, n_rays=None, white=False, no_dbg=False, det=False, no_part=False, scale=(1.0, 1.0, 1.0), seed=0, raises=None):
    """mp_tr_composite_bwd (det: mp_tr_composite_bwd_det) on a case's numpy inputs.  d sdf[p] and d rgb[p] cover the person's
    rows plus GUARD_ROWS and a tail of TAIL floats; they, d bg_rgb and d beta start from a seeded pattern of the magnitudes
    `scale` = (d sdf, d rgb and d bg_rgb, d beta).  A missing rgb_values upstream is a zero tensor (the entry point reads it
    unconditionally), the other two are NULL.  white: bg_rgb NULL; no_dbg: d_bg_rgb NULL (its buffer is still returned).
    -> dict of numpy: d_sdf, d_rgb (lists), d_bg_rgb, d_beta, and the same with the suffix _0: the start values"""
    from multiply_amd import hip
    L = hip.lib()
    R, P, NZ = c["shape"]
    rs = np.random.RandomState(seed)
    tabs, keep = _tables(c, ("inv", "z", "sdf", "rgb"))
    beta_d = torch.tensor([c["beta"]], dtype=torch.float32, device="cuda")
    bg = None if white else _dev(c["bg"])
    start = dict(d_sdf=[(rs.randn((s.shape[0] + GUARD_ROWS) * s.shape[1] + TAIL) * scale[0]).astype(np.float32) for s in c["sdf"]],
                 d_rgb=[(rs.randn((s.shape[0] + GUARD_ROWS) * s.shape[1] * 3 + TAIL) * scale[1]).astype(np.float32) for s in c["sdf"]],
                 d_bg_rgb=(rs.randn(R, 3) * scale[1]).astype(np.float32), d_beta=np.array([rs.randn() * scale[2]], np.float32))
    d_sdf, d_rgb = [_dev(b.copy()) for b in start["d_sdf"]], [_dev(b.copy()) for b in start["d_rgb"]]
    d_bg, d_beta = _dev(start["d_bg_rgb"].copy()), _dev(start["d_beta"].copy())
    t_dsdf = hip.device_ints([t.data_ptr() for t in d_sdf], "cuda")
    t_drgb = hip.device_ints([t.data_ptr() for t in d_rgb], "cuda")
    g_rgb = _dev(np.zeros((R, 3), np.float32) if up.get("rgb_values") is None else np.asarray(up["rgb_values"], dtype=np.float32))
    g_acc = None if up.get("acc") is None else _dev(np.asarray(up["acc"], dtype=np.float32))
    g_accp = None if up.get("acc_person") is None else _dev(np.asarray(up["acc_person"], dtype=np.float32))
    args = (R if n_rays is None else n_rays, P, NZ, *tabs, beta_d, bg, g_rgb, g_acc, g_accp, t_dsdf, t_drgb,
            None if no_dbg else d_bg, d_beta)
    if det:
        part = None if no_part else torch.full((R,), POISON, dtype=torch.float32, device="cuda")
        _call(L.mp_tr_composite_bwd_det, (*args, part, hip.stream()), raises)
    else:
        _call(L.mp_tr_composite_bwd, (*args, hip.stream()), raises)
    out = dict(d_sdf=[t.cpu().numpy() for t in d_sdf], d_rgb=[t.cpu().numpy() for t in d_rgb], d_bg_rgb=d_bg.cpu().numpy(),
               d_beta=float(d_beta.cpu()[0]))
    out.update({k + "_0": v for k, v in start.items()})
    out["d_beta_0"] = float(start["d_beta"][0])
    return out


def unchanged(out):
    """no buffer of a backward launch was written"""
    return (all(np.array_equal(a, b) for k in ("d_sdf", "d_rgb") for a, b in zip(out[k], out[k + "_0"]))
            and np.array_equal(out["d_bg_rgb"], out["d_bg_rgb_0"]) and out["d_beta"] == out["d_beta_0"])


def _used_rows(c, n, n_rays):
    """mask over person n's padded table rows: the rows a ray below n_rays refers to"""
    used = np.zeros(c["sdf"][n].shape[0] + GUARD_ROWS, bool)
    iv = np.asarray(c["inv"][n])[:n_rays]
    used[iv[iv >= 0]] = True
    return used


# ------------------------------------------------------------------------------------------------ comparisons
def compare_forward(tag, got, ref, c, n_rays=None, white=False):
    """every output per element against the float64 reference; exact values on missed persons and rays without samples;
    the rows past n_rays keep their poison -> {output: its largest error}"""
    R, P, NZ = c["shape"]
    n = R if n_rays is None else n_rays
    hit = np.stack([np.asarray(iv) >= 0 for iv in c["inv"]], 1)[:n]
    errs = {}
    for k in FWD:
        g = got[k].astype(np.float64)
        assert np.isfinite(g[:n]).all(), (tag, k)
        assert (got[k][n:] == POISON).all(), (tag, k)
        errs[k] = float(np.abs(g[:n] - ref[k][:n]).max()) if n else 0.0
        _note(f"forward {k}", errs[k] / TOL.scaled(1.0, NZ - 1))
    print(f"[composite] forward {tag}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    for k in FWD:
        assert errs[k] <= TOL.scaled(TOL.OUT[k], NZ - 1), (tag, k, errs[k])
    assert (got["acc_person"][:n][~hit] == 0).all(), tag
    none = ~hit.any(1)
    bg = np.ones((R, 3), np.float32) if white else c["bg"]
    assert np.array_equal(got["rgb_values"][:n][none], bg[:n][none]) and (got["fg_rgb_values"][:n][none] == 1).all(), tag
    assert (got["acc"][:n][none] == 0).all() and (got["normal_values"][:n][none] == 0).all() and (got["bg_T"][:n][none] == 1).all(), tag
    return errs


def compare_backward(tag, out, want, c, full=None, n_rays=None, thin=None, white=False, no_dbg=False):
    """a backward launch against float64 gradients `want`; the scales are those of `full` (the case with all three upstream
    gradients; default: want).  thin: the forward reference's bg_T, for the restricted measure.  Rows no ray below n_rays
    refers to, guard rows, tails and d bg_rgb past n_rays must be bit-unchanged.
    -> dict of the measures"""
    R, P, NZ = c["shape"]
    S = NZ - 1
    n = R if n_rays is None else n_rays
    full = want if full is None else full
    top_c = float(np.abs(c["up"]["rgb_values"]).max())
    got_sdf, got_rgb, masks = [], [], []
    for p in range(P):
        rows = c["sdf"][p].shape[0]
        used = _used_rows(c, p, n)
        for key, width, dest in (("d_sdf", S, got_sdf), ("d_rgb", 3 * S, got_rgb)):
            a, b = out[key][p], out[key + "_0"][p]
            body = (rows + GUARD_ROWS) * width
            a2, b2 = a[:body].reshape(-1, width), b[:body].reshape(-1, width)
            assert np.isfinite(a).all(), (tag, key, p)
            assert np.array_equal(a2[~used], b2[~used]), (tag, key, p, "rows no ray refers to")
            assert np.array_equal(a[body:], b[body:]), (tag, key, p, "tail")
            dest.append(a2[:rows].astype(np.float64))
        masks.append(np.repeat(used[:rows, None], S, 1))
    m = {}
    m["dsdf"] = CR.abs_error(got_sdf, want["d_sdf"], masks) / CR.top_of(full["d_sdf"])
    if thin is not None:
        sub = [a & b for a, b in zip(CR.thin_subset(c["inv"], c["sdf"], thin), masks)]
        m["dsdf_thin"] = CR.abs_error(got_sdf, want["d_sdf"], sub) / CR.top_of(full["d_sdf"], sub)
    m["drgb"] = max(float(np.abs(g.reshape(-1, S, 3) - w)[k].max()) for g, w, k in zip(got_rgb, want["d_rgb"], masks) if k.any()) / top_c
    if no_dbg:
        assert np.array_equal(out["d_bg_rgb"], out["d_bg_rgb_0"]), (tag, "d bg_rgb was never handed over")
    else:
        assert np.array_equal(out["d_bg_rgb"][n:], out["d_bg_rgb_0"][n:]), (tag, "d bg_rgb past n_rays")
        w_bg = want["d_bg_rgb"] if want["d_bg_rgb"] is not None else None
        if w_bg is not None:
            m["dbg"] = float(np.abs(out["d_bg_rgb"][:n].astype(np.float64) - w_bg[:n]).max()) / top_c if n else 0.0
    rays = want["d_beta_rays"][:n]
    w_beta, sum_abs = float(rays.sum()), float(np.abs(full["d_beta_rays"][:n]).sum())
    f_beta = abs(float(full["d_beta_rays"][:n].sum()))
    m["dbeta"] = abs((out["d_beta"] - out["d_beta_0"]) - w_beta) / (f_beta if f_beta >= 0.1 * sum_abs else sum_abs)
    for k, v in m.items():
        _note(f"backward {k}", v / TOL.scaled(1.0, S))
    print(f"[composite] backward {tag}: " + ", ".join(f"{k} {v:.3e}" for k, v in m.items()) +
          f" (max |d sdf| {CR.top_of(full['d_sdf']):.3e}, d beta {w_beta:.3e})")
    return m


def within(m, S):
    bounds = dict(dsdf=TOL.DSDF, dsdf_thin=TOL.DSDF_THIN, drgb=TOL.DRGB, dbg=TOL.DBG, dbeta=TOL.DBETA)
    return all(v <= TOL.scaled(bounds[k], S) for k, v in m.items())


def _scales(c, grad):
    """start patterns of a quarter of the gradient's own magnitudes"""
    top = max(float(np.abs(a).max()) for a in grad["d_sdf"])
    return 0.25 * top, 0.25 * float(np.abs(c["up"]["rgb_values"]).max()), 0.25 * abs(grad["d_beta"])


def _constructed_reference(c, white=False):
    R = c["shape"][0]
    bg = None if white else c["bg"]
    fwd = CR.composite_reference(R, c["inv"], c["z"], c["sdf"], c["rgb"], c["nrm"], c["beta"], bg)
    grad = CR.autograd_gradients(R, c["inv"], c["z"], c["sdf"], c["rgb"], c["beta"], bg, c["up"])
    return fwd, grad


# ------------------------------------------------------------------------------------------------ 1. kernels vs float64
@pytest.mark.parametrize("name", [c[0] for c in CR.CASES])
def test_forward_against_the_float64_reference(name):
    c, ref, _, _ = CR.reference(name)
    got = forward(c, guard=3)
    compare_forward(name, got, ref, c)
    again = forward(c, guard=3)                                   # no atomics: bit-identical from run to run
    assert all(np.array_equal(got[k], again[k]) for k in FWD)
    _report()


@pytest.mark.parametrize("name", [c[0] for c in CR.CASES])
def test_backward_against_float64_autograd(name):
    c, ref, grad, up = CR.reference(name)
    out = backward(c, up, scale=_scales(c, grad))
    m = compare_backward(name, out, grad, c, thin=ref["bg_T"] if c["regime"] == "thin" else None)
    _report()
    assert within(m, c["shape"][2] - 1), m


@pytest.mark.parametrize("name", ["thin-70x3", "opaque-9x2", "thin-13x8", "tiny-6x2-thin"])
def test_the_deterministic_form_gives_the_same(name):
    """d sdf, d rgb and d bg_rgb never went through atomics: bit-equal; d beta within the same bound (its summation order is
    tests/test_deterministic_sums_gpu.py's subject)"""
    c, ref, grad, up = CR.reference(name)
    plain = backward(c, up, scale=_scales(c, grad), seed=5)
    det = backward(c, up, scale=_scales(c, grad), seed=5, det=True)
    for k in ("d_sdf", "d_rgb"):
        assert all(np.array_equal(a, b) for a, b in zip(plain[k], det[k])), k
    assert np.array_equal(plain["d_bg_rgb"], det["d_bg_rgb"])
    m = compare_backward(name + " det", det, grad, c, thin=ref["bg_T"] if c["regime"] == "thin" else None)
    assert within(m, c["shape"][2] - 1), m


# ------------------------------------------------------------------------------------------------ 2. constructed rows
def test_constructed_rows_tied_depths():
    """(a) two persons with identical depth rows: every t_end ties and the lower column goes first"""
    c = CR.tied_rows()
    R, P, NZ = c["shape"]
    ref, grad = _constructed_reference(c)
    got = forward(c)
    compare_forward("tied rows", got, ref, c)
    swapped = CR.composite_reference(R, c["inv"], c["z"], c["sdf"][::-1], c["rgb"][::-1], c["nrm"][::-1], c["beta"], c["bg"])
    assert np.abs(swapped["acc_person"][:, ::-1] - ref["acc_person"]).max() > 1e-2       # what 'higher column first' would give
    assert np.abs(got["acc_person"] - ref["acc_person"]).max() <= TOL.OUT["acc_person"]
    m = compare_backward("tied rows", backward(c, c["up"], scale=_scales(c, grad)), grad, c, thin=ref["bg_T"])
    assert within(m, NZ - 1), m
    _report()


def test_constructed_rows_last_sample_tie():
    """(b) both persons end at the same final depth: the higher person's last sample is the last of the merged list, whichever
    of the two is dense; and rays whose larger final depth belongs to person 0 / person 1"""
    c = CR.last_tie_rows()
    R, P, NZ = c["shape"]
    ref, grad = _constructed_reference(c)
    other = CR.composite_reference(R, c["inv"], c["z"], c["sdf"], c["rgb"], c["nrm"], c["beta"], c["bg"], person_sign=-1)
    assert (np.abs(ref["bg_T"][:6] - other["bg_T"][:6]) > 1e-2).all()
    got = forward(c)
    compare_forward("last-sample tie", got, ref, c)
    print("[composite] last-sample tie: bg_T device", np.round(got["bg_T"], 4), "higher person last", np.round(ref["bg_T"], 4),
          "lower person last", np.round(other["bg_T"], 4))
    out = backward(c, c["up"], scale=_scales(c, grad))
    m = compare_backward("last-sample tie", out, grad, c, thin=ref["bg_T"])
    assert within(m, NZ - 1), m
    # the last samples alone, over their own maximum
    S = NZ - 1
    last = CR.last_samples(c["inv"], c["sdf"])
    e, top = CR.dsdf_error([a[:R * S].reshape(R, S) for a in out["d_sdf"]], grad["d_sdf"], last)
    _note("backward dsdf last samples of the tie rows", e)
    print(f"[composite] last-sample tie: d sdf of the last samples {e:.3e} of their max {top:.3e}")
    assert e <= TOL.DSDF_LAST
    _report()


def test_constructed_rows_zero_weights():
    """(c) beta = 0.001: an empty ray, an opaque first sample, repeated depths; colours and normals are NaN wherever fe == 0 and
    the forward must not read them.  (d) the adjoint reads every colour (the training step shades every sample: the header says
    so), so it runs on the same rows with finite colours."""
    c = CR.zero_weight_rows()
    R, P, NZ = c["shape"]
    ref = CR.composite_reference(R, c["inv"], c["z"], c["sdf"], c["rgb"], c["nrm"], c["beta"], c["bg"])
    got = forward(c)
    compare_forward("zero weights", got, ref, c)
    assert got["bg_T"][0] == 1 and got["acc"][0] == 0 and np.array_equal(got["rgb_values"][0], c["bg"][0])
    assert got["bg_T"][1] == 0 and got["acc_person"][1, 1] == 0
    fin = dict(c)
    rs = np.random.RandomState(5)
    fin["rgb"] = [np.where(np.isnan(a), rs.rand(*a.shape).astype(np.float32), a) for a in c["rgb"]]
    fin["nrm"] = [np.nan_to_num(a, nan=0.0) for a in c["nrm"]]
    fwd, grad = _constructed_reference(fin)
    assert all(np.array_equal(fwd[k], ref[k]) for k in FWD)                            # colours of weightless samples change nothing
    m = compare_backward("zero weights", backward(fin, fin["up"], scale=_scales(fin, grad)), grad, fin)
    assert within(m, NZ - 1), m
    _report()


# ------------------------------------------------------------------------------------------------ 3. NULL pointers
@pytest.mark.parametrize("name", ["thin-70x3", "opaque-9x2"])
def test_null_pointers(name):
    c, ref, grad, up = CR.reference(name)
    S = c["shape"][2] - 1
    thin = ref["bg_T"] if c["regime"] == "thin" else None
    sc = _scales(c, grad)
    # bg_rgb NULL: a white background, in both directions
    _, ref_w, grad_w, _ = CR.reference(name, white=True)
    compare_forward(name + " white", forward(c, white=True), ref_w, c, white=True)
    m = compare_backward(name + " white", backward(c, up, white=True, no_dbg=True, scale=sc), grad_w, c, thin=thin, no_dbg=True)
    assert within(m, S), m
    # every upstream gradient alone, errors over the whole case's scales; and all but d_acc / all but d_acc_person (the adjoint
    # is linear in the upstream gradients: the whole gradient minus that term's)
    minus = lambda a, b: dict(d_sdf=[x - y for x, y in zip(a["d_sdf"], b["d_sdf"])], d_rgb=[x - y for x, y in zip(a["d_rgb"], b["d_rgb"])],
                              d_bg_rgb=a["d_bg_rgb"] - b["d_bg_rgb"], d_beta=a["d_beta"] - b["d_beta"],
                              d_beta_rays=a["d_beta_rays"] - b["d_beta_rays"])
    for k in CR.UP_KEYS:
        _, _, g1, up1 = CR.reference(name, only=k)
        m = compare_backward(f"{name} only {k}", backward(c, up1, scale=sc), g1, c, full=grad, thin=thin)
        assert within(m, S), (k, m)
        if k != "rgb_values":
            rest = {j: (None if j == k else v) for j, v in up.items()}
            m = compare_backward(f"{name} without {k}", backward(c, rest, scale=sc), minus(grad, g1), c, full=grad, thin=thin)
            assert within(m, S), (k, m)
    # d_bg_rgb NULL: the buffer is never handed over; everything else is the full launch's, bit for bit
    a = backward(c, up, scale=sc, seed=9)
    b = backward(c, up, scale=sc, seed=9, no_dbg=True)
    assert np.array_equal(b["d_bg_rgb"], b["d_bg_rgb_0"])
    assert all(np.array_equal(x, y) for k in ("d_sdf", "d_rgb") for x, y in zip(a[k], b[k]))
    m = compare_backward(name + " no d_bg_rgb", b, grad, c, thin=thin, no_dbg=True)
    assert within(m, S), m
    _report()


# ------------------------------------------------------------------------------------------------ 4. launch shapes
@pytest.mark.parametrize("name", [c[0] for c in CR.LAUNCH_CASES])
def test_launch_shapes_of_the_adjoint(name):
    """P = 8: the adjoint runs 2 waves per block at S = 257 and 1 at S = 513 (bounds times S / 129); the forward's fixed 4 waves
    run at S = 257 and refuse S = 513 with -2 before any launch"""
    c, ref, grad, up = CR.reference(name)
    S = c["shape"][2] - 1
    m = compare_backward(name, backward(c, up, scale=_scales(c, grad)), grad, c, thin=ref["bg_T"])
    assert within(m, S), m
    det = backward(c, up, scale=_scales(c, grad), det=True)
    assert within(compare_backward(name + " det", det, grad, c, thin=ref["bg_T"]), S)
    if S == 513:
        got = forward(c, guard=1, raises=-2)
        assert all((got[k] == POISON).all() for k in FWD)
    else:
        compare_forward(name, forward(c, guard=1), ref, c)
    _report()


# ------------------------------------------------------------------------------------------------ 5. fewer rays, status codes
def test_fewer_rays_than_the_tables_hold():
    """n_rays = R - 3 (and 40, below RAGGED_HITS' last rays of person 1): forward rows past n_rays keep their poison, adjoint rows
    only later rays refer to stay bit-unchanged, everything else is the full launch's bit for bit; d beta is the sum of the
    first rays' own parts"""
    name = "thin-70x3"
    c, ref, grad, up = CR.reference(name)
    R, P, NZ = c["shape"]
    S = NZ - 1
    full_f = forward(c, guard=3)
    sc = _scales(c, grad)
    full_b = backward(c, up, scale=sc, seed=3)
    for n in (R - 3, 40):
        few = forward(c, n_rays=n, guard=3)
        compare_forward(f"{name} n_rays {n}", few, ref, c, n_rays=n)
        assert all(np.array_equal(few[k][:n], full_f[k][:n]) for k in FWD)
        out = backward(c, up, n_rays=n, scale=sc, seed=3)
        m = compare_backward(f"{name} n_rays {n}", out, grad, c, n_rays=n, thin=ref["bg_T"])
        assert within(m, S), m
        late = 0
        for p in range(P):
            used = _used_rows(c, p, n)[:c["sdf"][p].shape[0]]
            late += int((_used_rows(c, p, R)[:len(used)] & ~used).sum())
            for key, width in (("d_sdf", S), ("d_rgb", 3 * S)):
                a = out[key][p][:len(used) * width].reshape(-1, width)
                b = full_b[key][p][:len(used) * width].reshape(-1, width)
                assert np.array_equal(a[used], b[used]), (n, key, p)
        assert late > 0 or n == R - 3                              # (RAGGED_HITS: rays 65..69 are hit by nobody; below 40 by persons 0, 1)
        assert np.array_equal(out["d_bg_rgb"][:n], full_b["d_bg_rgb"][:n])


def test_argument_errors_make_no_launch():
    """-1: more than 8 persons; -2: the block does not fit the LDS; 0 for n_rays = 0; -3: the deterministic form without its
    scratch.  Nothing is written in any of them."""
    def dressed(R, P, NZ):
        inv, z, sdf = G.ragged_case(R, P, NZ, seed=1)
        return CR._dress(dict(name="status", shape=(R, P, NZ), beta=0.02, inv=inv, z=z, sdf=sdf), 1)
    c = dressed(5, 9, 34)
    assert all((v == POISON).all() for v in forward(c, guard=1, raises=-1).values())
    assert unchanged(backward(c, c["up"], raises=-1)) and unchanged(backward(c, c["up"], det=True, raises=-1))
    c = dressed(2, 8, 3000)                                       # one wave x 8 persons x 5 x 2999 floats of LDS
    assert all((v == POISON).all() for v in forward(c, raises=-2).values())
    assert unchanged(backward(c, c["up"], raises=-2)) and unchanged(backward(c, c["up"], det=True, raises=-2))
    c = dressed(5, 2, 34)
    assert all((v == POISON).all() for v in forward(c, n_rays=0, guard=1).values())
    assert unchanged(backward(c, c["up"], n_rays=0)) and unchanged(backward(c, c["up"], n_rays=0, det=True))
    assert unchanged(backward(c, c["up"], det=True, no_part=True, raises=-3))
    assert not unchanged(backward(c, c["up"], det=True))
