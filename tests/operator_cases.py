"""Inputs and comparison for the operator's ADMM kernels (csrc/operator_kernels.hip), one entry
point at a time: seeded input makers, one call on the numpy double of tests/fake_kernels.py and one
on the library, and the rounding bound the two are held to.  numpy only: importable without a GPU
(tests/test_operator_cases_ref.py checks the makers and the comparison there)."""
import numpy as np

from fake_kernels import FakeKernels, g0f

EPS = 2.0 ** -53
SENTINEL = -77.0          # what output arrays hold before the call: an element left unwritten shows
KAPPA = 5.0
VLO, VHI = -0.7, 1.1

# entry -> its arguments in header order (without the stream); "@name" is an array (None = NULL)
ARGS = {
    "revs_op_g0": "n T @pe @ps @gm kappa @g0",
    "revs_op_init_home": "n T @g0 @sb",
    "revs_op_init_node": "m T @cx @rho_v @bscale vlo vhi @zv @yv @w",
    "revs_aggregate_f32": "m T @node_ptr @inp @out",
    "revs_aggregate_f64": "m T @node_ptr @inp @scale @out",
    "revs_op_home_pass": "m T @node_ptr @isn @sb @g0 @xc @rho_b kappa alpha @rhat @cty @res",
    "revs_op_home_pass_fused": "m T @node_ptr @isn @sb @g0 @rho_b kappa alpha @rhat nslab @va @usa "
                               "@rho_v @bscale vlo vhi @xc @zv @yv @w",
    "revs_op_row_scale": "m T @s @inp @out",
    "revs_op_node_w": "m T @zv @yv @rho_v @w",
    "revs_op_node_scale": "m T nslab @ta @tb @s @rho_v @rho_b kappa @a @sa",
    "revs_op_node_update": "m T nslab @va @rhat @usa @rho_v @rho_b @bscale kappa alpha vlo vhi "
                           "@xc @zv @yv @w @res",
    "revs_op_export": "n T @sb @pe",
    "revs_op_node_prep": "m T @node_ptr @isn @pe @ps @gm kappa preclamp @p0 @gmin @g0_out",
    "revs_op_nodefast_feas": "m T nslab @v0 @bscale @gmin vlo vhi @cx @stats",
    "revs_op_nodefast_scale": "m T nslab @wh @ph0 @lam @rho_v kappa @xh @sx",
    "revs_op_nodefast_update": "m T nslab @zt @rho_v @bscale alpha vlo vhi @zv @yv @w @res",
    "revs_op_nodefast_dualres": "m T nslab @xh @ph0 @lam @yh kappa @res",
    "revs_op_nodefast_finish": "m T nslab @x @p0 @gmin @isn @d @slack @stats",
    "revs_op_node_apply": "m T @node_ptr @isn @pe @ps @gm kappa preclamp @d @pe_new",
}
ARGS = {k: v.split() for k, v in ARGS.items()}
# pointers an entry accepts as NULL
OPTIONAL = {"revs_op_init_node": {"bscale"}, "revs_aggregate_f64": {"scale"},
            "revs_op_home_pass": {"xc", "cty", "res"}, "revs_op_home_pass_fused": {"bscale"},
            "revs_op_node_update": {"bscale", "res"}, "revs_op_node_prep": {"g0_out"},
            "revs_op_nodefast_feas": {"bscale"}, "revs_op_nodefast_update": {"bscale", "res"}}


def lanes(T):
    """TL of the residence-shaped kernels: the power of two >= T among 32..256."""
    return 32 if T <= 32 else 64 if T <= 64 else 128 if T <= 128 else 256


def node_layout(T):
    """(node_ptr int64[m+1], inv_sqrt_n double[m]) over 20 nodes whose residence counts, unsorted,
    are 0 (first, last and in between), 1, HS-1, HS, HS+1, 2 HS + 3, 49, 130 with HS = 256 / TL(T)
    home lanes, and a few small ones.  inv_sqrt_n is 0 on the empty nodes, as the driver makes it."""
    hs = 256 // lanes(T)
    special = []
    for c in (49, 1, hs + 1, 130, hs - 1, 2 * hs + 3, hs):
        if c > 0 and c not in special:
            special.append(c)
    counts = [0] + special[:3] + [0] + special[3:]
    counts += [2, 0, 3, 1, 0, 5, 1, 2, 4, 3, 6, 2][:19 - len(counts)] + [0]
    counts = np.array(counts, np.int64)
    node_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    isn = np.where(counts > 0, 1.0 / np.sqrt(np.maximum(counts, 1)), 0.0)
    return node_ptr, isn


# ---------------------------------------------------------------- input makers
def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _out(shape, dt=np.float64):
    return np.full(shape, SENTINEL, dt)


def _slabs(rng, total, nslab):
    """`nslab` partial arrays, all different, that sum to about `total` (the callee's own sum is the
    truth; the last slab is what is left)."""
    parts = [rng.normal(0, 2.0, total.shape) for _ in range(nslab - 1)]
    return np.ascontiguousarray(np.stack(parts + [total - sum(parts)]))


def _clip_targets(rng, shape, bs, vlo, vhi):
    """Values of which a third each ends below bs vlo, above bs vhi and strictly inside."""
    kind = rng.integers(0, 3, shape)
    lo, hi = bs * vlo * np.ones(shape), bs * vhi * np.ones(shape)
    inside = lo + rng.uniform(0.1, 0.9, shape) * (hi - lo)
    return np.where(kind == 0, lo - rng.uniform(0.5, 3, shape),
                    np.where(kind == 1, hi + rng.uniform(0.5, 3, shape), inside))


def _jitter_isn(rng, isn):
    """inv_sqrt_n all different (nodes with equal counts included); still 0 on the empty nodes."""
    return isn * rng.uniform(0.8, 1.25, isn.shape)


def _float_state(rng, n, T):
    f = np.float32
    return dict(pe=rng.uniform(0, 4, (n, T)).astype(f), ps=rng.uniform(0, 4, (n, T)).astype(f),
                gm=rng.normal(0, 9, (n, T)).astype(f))


def _prefill_res(entry, arrays, scalars, rows, rng):
    """res with some entries above and some below what the call produces on the touched `rows`,
    and arbitrary positive values on the others."""
    T = scalars["T"]
    trial = dict(arrays, res=np.zeros((8, T)))
    new = run_fake(entry, trial, scalars)["res"]
    res = rng.uniform(0.5, 3.0, (8, T))
    for r in rows:
        res[r] = new[r] * rng.choice([0.5, 2.0], T)
    arrays["res"] = res


def make_g0(n, T):
    rng = _rng(1, n, T)
    return dict(_float_state(rng, n, T), g0=_out((n, T))), dict(n=n, T=T, kappa=KAPPA)


def make_init_home(n, T):
    rng = _rng(2, n, T)
    return dict(g0=rng.normal(0, 3, (n, T)), sb=_out((n, T))), dict(n=n, T=T)


def make_export(n, T):
    rng = _rng(3, n, T)
    return dict(sb=rng.normal(0, 3, (n, T)), pe=_out((n, T), np.float32)), dict(n=n, T=T)


def make_aggregate(T, integer):
    rng = _rng(4, T, integer)
    node_ptr, _ = node_layout(T)
    m, n = len(node_ptr) - 1, int(node_ptr[-1])
    x = rng.integers(-8, 9, (n, T)) if integer else rng.normal(0, 3, (n, T))
    return (dict(node_ptr=node_ptr, inp=x.astype(np.float32), out=_out((m, T), np.float32)),
            dict(m=m, T=T))


def _node_common(rng, M, T, bscale_on):
    return dict(rho_v=rng.uniform(0.5, 2.0, T), rho_b=rng.uniform(0.5, 2.0, T),
                bscale=rng.uniform(0.5, 2.5, M) if bscale_on else None)


def make_init_node(M, T, bscale_on=True):
    rng = _rng(5, M, T, bscale_on)
    c = _node_common(rng, M, T, bscale_on)
    bs = c["bscale"][:, None] if bscale_on else 1.0
    a = dict(cx=_clip_targets(rng, (M, T), bs, VLO, VHI), rho_v=c["rho_v"], bscale=c["bscale"],
             zv=_out((M, T)), yv=_out((M, T)), w=_out((M, T)))
    return a, dict(m=M, T=T, vlo=VLO, vhi=VHI)


def make_row_scale(M, T):
    rng = _rng(6, M, T)
    return (dict(s=rng.uniform(0.1, 3.0, M), inp=rng.normal(0, 3, (M, T)), out=_out((M, T))),
            dict(m=M, T=T))


def make_node_w(M, T):
    rng = _rng(7, M, T)
    return (dict(zv=rng.normal(0, 2, (M, T)), yv=rng.normal(0, 2, (M, T)),
                 rho_v=rng.uniform(0.5, 2.0, T), w=_out((M, T))), dict(m=M, T=T))


def make_node_scale(M, T, nslab):
    rng = _rng(8, M, T, nslab)
    c = _node_common(rng, M, T, False)
    a = dict(ta=rng.normal(0, 2, (nslab, M, T)), tb=rng.normal(0, 2, (nslab, M, T)),
             s=rng.uniform(0.1, 3.0, M), rho_v=c["rho_v"], rho_b=c["rho_b"], a=_out((M, T)),
             sa=_out((M, T)))
    return a, dict(m=M, T=T, nslab=nslab, kappa=KAPPA)


def _zy_update_inputs(rng, M, T, nslab, bscale_on, alpha):
    """z_v, y_v, rho_v, bound_scale and the slabs of zt such that clip(alpha zt + (1-alpha) z_v +
    y_v / rho_v) ends a third each at either bound and inside."""
    c = _node_common(rng, M, T, bscale_on)
    bs = c["bscale"][:, None] if bscale_on else 1.0
    zv, yv = rng.normal(0, 2, (M, T)), rng.normal(0, 2, (M, T))
    target = _clip_targets(rng, (M, T), bs, VLO, VHI)
    zt = (target - yv / c["rho_v"][None, :] - (1 - alpha) * zv) / alpha
    return c, zv, yv, _slabs(rng, zt, nslab)


def make_node_update(M, T, nslab=1, bscale_on=True, res=None, alpha=1.6, seed=0):
    rng = _rng(9, M, T, nslab, bscale_on, res is not None, int(alpha * 10), seed)
    c, zv, yv, usa = _zy_update_inputs(rng, M, T, nslab, bscale_on, alpha)
    a = dict(va=_slabs(rng, rng.normal(0, 3, (M, T)), nslab), rhat=rng.normal(0, 3, (M, T)), usa=usa,
             rho_v=c["rho_v"], rho_b=c["rho_b"], bscale=c["bscale"], xc=_out((M, T)), zv=zv, yv=yv,
             w=_out((M, T)), res=None)
    s = dict(m=M, T=T, nslab=nslab, kappa=KAPPA, alpha=alpha, vlo=VLO, vhi=VHI)
    if res == "fill":
        _prefill_res("revs_op_node_update", a, s, (0, 3, 4), rng)
    return a, s


def make_nodefast_scale(M, T, nslab):
    rng = _rng(10, M, T, nslab)
    a = dict(wh=rng.normal(0, 2, (nslab, M, T)), ph0=rng.normal(0, 3, (M, T)),
             lam=rng.uniform(0.1, 3.0, M), rho_v=rng.uniform(0.5, 2.0, T), xh=_out((M, T)),
             sx=_out((M, T)))
    return a, dict(m=M, T=T, nslab=nslab, kappa=KAPPA)


def make_nodefast_update(M, T, nslab=1, bscale_on=True, res=None, alpha=1.6):
    rng = _rng(11, M, T, nslab, bscale_on, res is not None, int(alpha * 10))
    c, zv, yv, zt = _zy_update_inputs(rng, M, T, nslab, bscale_on, alpha)
    a = dict(zt=zt, rho_v=c["rho_v"], bscale=c["bscale"], zv=zv, yv=yv, w=_out((M, T)), res=None)
    s = dict(m=M, T=T, nslab=nslab, alpha=alpha, vlo=VLO, vhi=VHI)
    if res == "fill":
        _prefill_res("revs_op_nodefast_update", a, s, (0, 3, 4), rng)
    return a, s


def make_nodefast_dualres(M, T, nslab=1, res="zero"):
    rng = _rng(12, M, T, nslab, res == "fill")
    a = dict(xh=rng.normal(0, 3, (M, T)), ph0=rng.normal(0, 3, (M, T)), lam=rng.uniform(0.1, 3.0, M),
             yh=rng.normal(0, 2, (nslab, M, T)), res=np.zeros((8, T)))
    s = dict(m=M, T=T, nslab=nslab, kappa=KAPPA)
    if res == "fill":
        _prefill_res("revs_op_nodefast_dualres", a, s, (2, 5, 6, 7), rng)
    return a, s


def _stats(fill):
    return np.zeros(2) if fill == "zero" else np.array([1.0e3, 2.0e3])


def make_nodefast_feas(M, T, nslab=1, bscale_on=True, violate=True, stats="zero"):
    rng = _rng(13, M, T, nslab, bscale_on, violate, stats == "zero")
    bsv = rng.uniform(0.5, 2.5, M) if bscale_on else None
    bs = bsv[:, None] if bscale_on else 1.0
    if violate:
        v = _clip_targets(rng, (M, T), bs, VLO, VHI)
        gmin = rng.normal(0, 2, (M, T))
    else:
        v = bs * (VLO + rng.uniform(0.1, 0.9, (M, T)) * (VHI - VLO))
        gmin = rng.uniform(0.1, 3.0, (M, T))
    gmin[rng.integers(0, M)] = np.inf                 # an empty node
    a = dict(v0=_slabs(rng, v, nslab), bscale=bsv, gmin=gmin, cx=_out((M, T)), stats=_stats(stats))
    return a, dict(m=M, T=T, nslab=nslab, vlo=VLO, vhi=VHI)


def make_nodefast_finish(M, T, nslab=1, violate=True, stats="zero"):
    rng = _rng(14, M, T, nslab, violate, stats == "zero")
    x, p0 = rng.normal(0, 3, (M, T)), rng.normal(0, 3, (M, T))
    isn = rng.uniform(0.1, 1.0, M)
    empty = rng.integers(0, M)
    isn[empty] = 0.0
    xs = _slabs(rng, x, nslab)
    dv = xs.sum(axis=0) - p0
    gmin = rng.normal(0, 1, (M, T)) if violate else np.abs(isn[:, None] * dv) + rng.uniform(0.1, 1, (M, T))
    gmin[empty] = np.inf
    a = dict(x=xs, p0=p0, gmin=gmin, isn=isn, d=_out((M, T)), slack=_out((M, T)), stats=_stats(stats))
    return a, dict(m=M, T=T, nslab=nslab)


def _home_arrays(rng, T):
    node_ptr, isn = node_layout(T)
    m, n = len(node_ptr) - 1, int(node_ptr[-1])
    return m, n, dict(node_ptr=node_ptr, isn=_jitter_isn(rng, isn), sb=rng.normal(0, 2, (n, T)),
                      g0=rng.normal(0.5, 2, (n, T)))


def make_home_pass(T, form="res", alpha=1.6):
    """form: "rhs" (xc = NULL: only rhat), "upd" (update, no residuals), "res" (update with cty and
    a pre-filled res)."""
    rng = _rng(15, T, ["rhs", "upd", "res"].index(form), int(alpha * 10))
    m, n, a = _home_arrays(rng, T)
    a.update(xc=None if form == "rhs" else rng.normal(0, 1.5, (m, T)), rho_b=rng.uniform(0.5, 2.0, T),
             rhat=_out((m, T)), cty=rng.normal(0, 2, (m, T)) if form == "res" else None, res=None)
    s = dict(m=m, T=T, kappa=KAPPA, alpha=alpha)
    if form == "res":
        _prefill_res("revs_op_home_pass", a, s, (1, 2, 5, 6, 7), rng)
    return a, s


def make_home_pass_fused(T, nslab=1, bscale_on=True, alpha=1.6):
    rng = _rng(16, T, nslab, bscale_on, int(alpha * 10))
    m, n, a = _home_arrays(rng, T)
    nu, s = make_node_update(m, T, nslab, bscale_on, None, alpha, seed=16)
    del nu["res"]
    a.update(nu)
    return a, s


def make_node_prep(T, preclamp=0, g0_out_on=True):
    rng = _rng(17, T, preclamp, g0_out_on)
    m, n, h = _home_arrays(rng, T)
    a = dict(node_ptr=h["node_ptr"], isn=h["isn"], **_float_state(rng, n, T), p0=_out((m, T)),
             gmin=_out((m, T)), g0_out=_out((n, T)) if g0_out_on else None)
    return a, dict(m=m, T=T, kappa=KAPPA, preclamp=preclamp)


def make_node_apply(T, preclamp=0, dzero=False):
    rng = _rng(18, T, preclamp, dzero)
    m, n, h = _home_arrays(rng, T)
    a = dict(node_ptr=h["node_ptr"], isn=h["isn"], **_float_state(rng, n, T),
             d=np.zeros((m, T)) if dzero else rng.normal(0, 1, (m, T)), pe_new=_out((n, T), np.float32))
    return a, dict(m=m, T=T, kappa=KAPPA, preclamp=preclamp)


# ---------------------------------------------------------------- running an entry
def _call(impl, calls, arrays, pointer):
    for entry, scalars in calls:
        args = [pointer(arrays.get(tok[1:])) if tok[0] == "@" else scalars[tok] for tok in ARGS[entry]]
        rc = getattr(impl, entry)(*args, None)
        assert rc == 0, (entry, rc, impl.revs_last_error())


def run_fake(entry, arrays, scalars, fake=None):
    """One call of `entry` on the numpy double over host copies; every array afterwards."""
    host = {k: None if v is None else np.ascontiguousarray(v).copy() for k, v in arrays.items()}
    _call(fake or FakeKernels(), [(entry, scalars)], host, lambda a: None if a is None else a.ctypes.data)
    return host


def run_lib_seq(lib, calls, arrays):
    """The calls [(entry, scalars), ...] on the library, in order, over ONE set of device copies."""
    import torch
    dev = {k: None if v is None else torch.from_numpy(np.ascontiguousarray(v).copy()).to("cuda:0")
           for k, v in arrays.items()}
    _call(lib, calls, dev, lambda t: None if t is None else t.data_ptr())
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in dev.items()}


def run_both(entry, arrays, scalars, lib=None, fake=None):
    """(reference, got): `entry` once on FakeKernels over host copies and, with a library (the GPU
    machine), once on it over device copies.  Both hold EVERY array after the call, inputs included;
    `got` is None without a library."""
    ref = run_fake(entry, arrays, scalars, fake)
    got = None if lib is None else run_lib_seq(lib, [(entry, scalars)], arrays)
    return ref, got


# ---------------------------------------------------------------- the comparison
def close(got, ref, S, chain):
    """|got - ref| <= 2 (chain + 8) 2^-53 S, elementwise.  S: the reference expression with every term
    replaced by its absolute value; chain: additions in the longest sum.  Both sides round each
    operation once (2^-53 relative); the factor 2 is for the two sides, 8 for the operations around
    the sum.  Where the reference is not finite (gmin = +inf of an empty node) equality is owed."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return False
    with np.errstate(invalid="ignore"):
        ok = np.where(np.isfinite(ref), np.abs(got - ref) <= 2.0 * (chain + 8.0) * EPS * S, got == ref)
    return bool(np.all(ok))


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _counts(a):
    return np.diff(a["node_ptr"])


def _seg_sum(a, x):
    m = len(a["node_ptr"]) - 1
    out = np.zeros((m, x.shape[1]))
    np.add.at(out, np.repeat(np.arange(m), _counts(a)), x)
    return out


def _seg_max(a, x):
    """per-slot maximum over all residences (zeros when there are none)"""
    return x.max(axis=0) if x.shape[0] else np.zeros(x.shape[1])


def _bs(a):
    return a["bscale"][:, None] if a.get("bscale") is not None else 1.0


def _res_S(a, rows):
    """S of res: the larger of what was there and of the new maxima's S on the touched rows, 0 (bit
    equality with the reference, which leaves them alone) on the others."""
    S = np.zeros_like(a["res"])
    for r, val in rows.items():
        S[r] = np.maximum(a["res"][r], val)
    return S


def _zy_S(a, s, zt_slabs):
    """S of z_v, y_v, w (and of res rows 0, 3, 4) of the node update from the slabs of zt."""
    rv, al = a["rho_v"][None, :], s["alpha"]
    azt = np.abs(zt_slabs).sum(axis=0)
    Sh = al * azt + abs(1 - al) * np.abs(a["zv"])
    Sz = np.maximum(Sh + np.abs(a["yv"]) / rv, _bs(a) * max(abs(s["vlo"]), abs(s["vhi"])))
    Sy = np.abs(a["yv"]) + rv * (Sh + Sz)
    out = dict(zv=(Sz, s["nslab"]), yv=(Sy, s["nslab"]), w=(rv * Sz + Sy, s["nslab"]))
    if a.get("res") is not None:
        out["res"] = (_res_S(a, {0: (azt + Sz).max(axis=0), 3: azt.max(axis=0), 4: Sz.max(axis=0)}),
                      s["nslab"])
    return out


def _home_S(a, s, Sxc, chain0):
    """S of sb, rhat and res rows 1, 2, 5, 6, 7 of the home pass; Sxc = S of the node correction (None:
    no update); chain0 = additions behind xc."""
    k, al, rb = s["kappa"], s["alpha"], a["rho_b"][None, :]
    node = np.repeat(np.arange(len(a["isn"])), _counts(a))
    isn = a["isn"][:, None]
    aG, Z, Y = np.abs(a["g0"]), np.maximum(a["sb"], 0), -np.minimum(a["sb"], 0)
    out = {}
    if Sxc is not None:
        Sxt = (k * aG + rb * Z + Y) / (k + rb) + (isn * Sxc)[node]
        Su = al * Sxt + abs(1 - al) * Z + Y / rb
        Z, Y = Su, rb * Su
        out["sb"] = (Z + Y, chain0)
        if a.get("res") is not None:
            cy = (isn * np.abs(a["cty"]))[node] + Y
            out["res"] = (_res_S(a, {1: _seg_max(a, Sxt + Z), 2: _seg_max(a, k * (Sxt + aG) + cy),
                                     5: _seg_max(a, Sxt), 6: _seg_max(a, cy), 7: _seg_max(a, k * aG)}),
                          chain0)
    out["rhat"] = (isn * _seg_sum(a, k * aG + rb * Z + Y), _counts(a)[:, None] + chain0)
    return out


def bounds(entry, a, s):
    """name -> (S, chain) of every array `entry` writes, from the inputs `a` as they were BEFORE the
    call.  S = 0 asks for the reference's bits.  ("ulp32",) is the float rule of revs_op_node_apply."""
    e = entry.replace("revs_op_", "").replace("revs_", "")
    exact = lambda name: (np.zeros(a[name].shape), 0)
    if e == "g0":
        return dict(g0=exact("g0"))
    if e == "init_home":
        return dict(sb=exact("sb"))
    if e == "export":
        return dict(pe=exact("pe"))
    if e == "init_node":
        Sz = np.maximum(np.abs(a["cx"]), _bs(a) * max(abs(s["vlo"]), abs(s["vhi"])))
        return dict(zv=(Sz, 0), yv=exact("yv"), w=(a["rho_v"][None, :] * Sz, 0))
    if e == "row_scale":
        return dict(out=(np.abs(a["s"][:, None] * a["inp"]), 0))
    if e == "node_w":
        return dict(w=(a["rho_v"][None, :] * np.abs(a["zv"]) + np.abs(a["yv"]), 0))
    if e == "node_scale":
        sv = a["s"][:, None]
        Sa = (np.abs(a["ta"]).sum(axis=0) + sv * np.abs(a["tb"]).sum(axis=0)) / \
            (s["kappa"] + a["rho_b"][None, :] + a["rho_v"][None, :] * sv * sv)
        return dict(a=(Sa, s["nslab"]), sa=(sv * Sa, s["nslab"]))
    if e == "node_update":
        out = _zy_S(a, s, a["usa"])
        out["xc"] = (np.abs(a["va"]).sum(axis=0) + np.abs(a["rhat"]) / (s["kappa"] + a["rho_b"][None, :]),
                     s["nslab"])
        return out
    if e == "nodefast_update":
        return _zy_S(a, s, a["zt"])
    if e == "nodefast_scale":
        l = a["lam"][:, None]
        Sx = (s["kappa"] * np.abs(a["ph0"]) + l * np.abs(a["wh"]).sum(axis=0)) / \
            (s["kappa"] + a["rho_v"][None, :] * l * l)
        return dict(xh=(Sx, s["nslab"]), sx=(l * Sx, s["nslab"]))
    if e == "nodefast_dualres":
        k, ly = s["kappa"], a["lam"][:, None] * np.abs(a["yh"]).sum(axis=0)
        axh, aph = np.abs(a["xh"]), np.abs(a["ph0"])
        return dict(res=(_res_S(a, {2: (k * (axh + aph) + ly).max(axis=0), 5: axh.max(axis=0),
                                    6: ly.max(axis=0), 7: (k * aph).max(axis=0)}), s["nslab"]))
    if e == "nodefast_feas":
        av = np.abs(a["v0"]).sum(axis=0)
        S0 = (av + _bs(a) * max(abs(s["vlo"]), abs(s["vhi"]))).max()
        return dict(cx=(av, s["nslab"]), stats=(np.maximum(a["stats"], [S0, 0.0]), s["nslab"]))
    if e == "nodefast_finish":
        Sd = np.abs(a["x"]).sum(axis=0) + np.abs(a["p0"])
        with np.errstate(invalid="ignore"):
            Ss = np.abs(a["gmin"]) + a["isn"][:, None] * Sd
        S0 = Ss[np.isfinite(Ss)].max(initial=0.0)
        return dict(d=(Sd, s["nslab"]), slack=(Ss, s["nslab"]),
                    stats=(np.maximum(a["stats"], [S0, 0.0]), s["nslab"]))
    if e == "aggregate_f32":
        return dict(out=("f32sum",))
    if e == "node_prep":
        g = g0f(a["pe"], a["ps"], a["gm"], s["kappa"])
        out = dict(p0=(a["isn"][:, None] * _seg_sum(a, np.abs(g)), _counts(a)[:, None]),
                   gmin=exact("gmin"))
        if a.get("g0_out") is not None:
            out["g0_out"] = exact("g0_out")
        return out
    if e == "node_apply":
        return dict(pe_new=("ulp32",))
    if e == "home_pass":
        return _home_S(a, s, None if a.get("xc") is None else np.abs(a["xc"]), 0)
    if e == "home_pass_fused":
        out = bounds("revs_op_node_update", dict(a, res=None), s)
        out.update(_home_S(dict(a, res=None), s, out["xc"][0], s["nslab"]))
        return out
    raise KeyError(entry)


def compare(entry, before, scalars, ref, got):
    """Hold every array of `got` to `ref` after one call of `entry` on `before`: written arrays within
    their bound (bounds()), every other array bit for bit what it was.  Raises AssertionError naming
    the array; returns {"ulp32": number of float elements that used the one-ulp allowance}."""
    B = bounds(entry, before, scalars)
    used = {"ulp32": 0}
    for name, was in before.items():
        if was is None:
            assert got.get(name) is None, name
            continue
        g, r = got[name], ref[name]
        if name not in B:
            assert same_bits(g, np.ascontiguousarray(was)), f"{entry}: input {name} was changed"
        elif len(B[name]) == 1 and B[name][0] == "ulp32":
            # a double rounded to float: one float ulp, on at most 0.1 % of the elements
            diff = g != r
            assert np.all(np.abs(g.astype(np.float64) - r.astype(np.float64)) <= np.spacing(np.abs(r))), \
                f"{entry}: {name} off by more than one float ulp"
            assert diff.mean() <= 1e-3, f"{entry}: {name} differs on {diff.sum()} of {diff.size} elements"
            used["ulp32"] += int(diff.sum())
        elif len(B[name]) == 1 and B[name][0] == "f32sum":
            # float sums: chain 2^-24 sum|x| against the exact (double) sum
            x = before["inp"].astype(np.float64)
            exact, mag = _seg_sum(before, x), _seg_sum(before, np.abs(x))
            tol = _counts(before)[:, None] * 2.0 ** -24 * mag
            assert np.all(np.abs(g.astype(np.float64) - exact) <= tol), f"{entry}: {name}"
            assert np.all(np.abs(g.astype(np.float64) - r.astype(np.float64)) <= 2 * tol), f"{entry}: {name}"
        else:
            S, chain = B[name]
            assert close(g, r, S, chain), f"{entry}: {name} outside the rounding bound"
    return used
