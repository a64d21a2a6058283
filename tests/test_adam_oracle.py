"""The Adam oracle and its bound on the CPU: the f32 model of the kernel's formula stays inside the
bound in every hyperparameter case and contraction form (the bound is satisfiable), each wrong form
of the update misses it on a named case and output (the bound is sharp), and the host-device torch
path is held to the same oracle by the project's host rule."""
import numpy as np
import pytest
import torch

import adam_oracle as AO
import clip_oracle as CO

N = 20000


@pytest.mark.parametrize("scale", [None, 0.3])
@pytest.mark.parametrize("form", AO.FORMS)
def test_kernel_model_within_bound(form, scale):
    """Every element of p', m', v' of the f32 model, in every case: the reference alone is inside the
    bound, with the figure printed."""
    fig = AO.Figures()
    for name in AO.case_names():
        h, p, g, m, v = AO.make_case(name, N)
        if scale is not None:
            g = AO.scaled(g, scale)
        want, allowed, got = AO.oracle(p, g, m, v, h), AO.bound(p, g, m, v, h), AO.kernel_model(p, g, m, v, h, form)
        for k, out in enumerate("pmv"):
            fig.check(f"model {form} scale={scale} {name} {out}", got[k], want[k], allowed[k])
        band = slice(N - N // 8, N)
        hr, pb = AO.rounded(h), AO.a64(p)[band]
        assert np.all(np.isfinite(got[0])) and np.array_equal(want[0][band], pb - hr.lr * (0.0 + hr.wd * pb))
        assert not got[1][band].any() and not got[2][band].any()
    print(f"adam-figures model {form} scale={scale} worst " + " ".join(f"{k}={x:.3f}" for k, x in fig.worst.items()))
    fig.finish()


# ---------------------------------------------------------------------------- wrong forms (float64)
def _mutant(kind, p, g, m, v, h, g_raw=None):
    h = AO.rounded(h)
    p, g, m, v = AO.a64(p), AO.a64(g), AO.a64(m), AO.a64(v)
    lr, b1, b2, eps, wd, t = h
    gm = gv = g
    omb1 = 1.0 - b1
    if kind == "coupled_l2":
        gm = gv = g + wd * p
    if kind == "v_from_unscaled_grad":
        gv = AO.a64(g_raw)
    if kind == "one_minus_b1_as_0.1":
        omb1 = 0.1
    if kind == "count_minus_1":
        t = t - 1
    m2 = b1 * m + omb1 * gm
    v2 = b2 * v + (1.0 - b2) * gv * gv
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "eps_scaled_with_root":
            q = (m2 / bc1) / ((np.sqrt(v2) + eps) / np.sqrt(bc2))
        else:
            q = (m2 / bc1) / (np.sqrt(v2 / bc2) + eps)
        if kind == "decay_on_updated_p":
            p2 = p - lr * q
            p2 = p2 - lr * wd * p2
        elif kind == "coupled_l2":
            p2 = p - lr * q
        elif kind == "update_times_1+2^-10":
            p2 = p - lr * (q + wd * p) * (1.0 + 2.0 ** -10)
        else:
            p2 = p - lr * (q + wd * p)
    return p2, m2, v2


MUTANTS = [  # (wrong form, case, clip scale, the output that must miss)
    ("eps_scaled_with_root", "eps/wd=0", None, "p"),
    ("eps_scaled_with_root", "eps/wd=0.1", None, "p"),
    ("decay_on_updated_p", "large_count/wd=0.1", None, "p"),
    ("coupled_l2", "warm/wd=0.1", None, "m"),
    ("coupled_l2", "warm/wd=0.1", None, "v"),
    ("coupled_l2", "warm/wd=0.1", None, "p"),
    ("count_minus_1", "fresh/wd=0", None, "p"),
    ("count_minus_1", "warm/wd=0", None, "p"),
    ("count_minus_1", "large_count/wd=0", None, "p"),
    ("update_times_1+2^-10", "warm/wd=0", None, "p"),
    ("update_times_1+2^-10", "large_count/wd=0.1", None, "p"),
    ("v_from_unscaled_grad", "warm/wd=0", 0.3, "v"),
    ("v_from_unscaled_grad", "warm/wd=0", 0.3, "p"),
    ("one_minus_b1_as_0.1", "fresh/wd=0", None, "m"),
    ("one_minus_b1_as_0.1", "warm/wd=0.1", None, "m"),
]


@pytest.mark.parametrize("kind,case,scale,out", MUTANTS)
def test_wrong_forms_miss_the_bound(kind, case, scale, out):
    """Each wrong form, evaluated exactly (float64), is outside the bound of the named output on the
    named case -- at more than one element in a hundred, so a kernel with that error cannot pass."""
    h, p, g_raw, m, v = AO.make_case(case, N)
    g = AO.scaled(g_raw, scale) if scale is not None else g_raw
    want, allowed = AO.oracle(p, g, m, v, h), AO.bound(p, g, m, v, h)
    got = _mutant(kind, p, g, m, v, h, g_raw)
    k = "pmv".index(out)
    live = slice(0, N - N // 8)                 # outside the zero band
    err = np.abs(got[k] - want[k])[live]
    miss = ~(err < allowed[k][live])            # (a NaN misses)
    with np.errstate(invalid="ignore"):
        worst = np.nanmax(np.where(np.isfinite(err), err / allowed[k][live], np.inf))
    print(f"adam-figures mutant {kind} {case} scale={scale} {out} missing={miss.mean():.3f} worst_fraction_of_bound={worst:.1f}")
    assert miss.mean() > 0.01, (kind, case, out, miss.mean(), worst)


def test_zero_band_is_exact_decay():
    """g = m = v = 0: the oracle is p (1 - lr wd) with no NaN and the bound there is a few u |p|."""
    h, p, g, m, v = AO.make_case("warm/wd=0.1", 64)
    hr = AO.rounded(h)
    want, allowed = AO.oracle(p, g, m, v, h), AO.bound(p, g, m, v, h)
    band = slice(56, 64)
    p64 = AO.a64(p)[band]
    np.testing.assert_allclose(want[0][band], p64 * (1.0 - hr.lr * hr.wd), rtol=1e-15)
    assert not want[1][band].any() and not want[2][band].any()
    assert np.all(allowed[0][band] <= 3 * AO.U * np.abs(p64)) and np.all(allowed[0][band] > 0)
    assert np.all(allowed[1][band] <= 2 * AO.ETA) and np.all(allowed[2][band] <= 2 * AO.ETA)


def test_launch_tiles_rule():
    t = lambda R, C, vec=True, mx=False, S=0: dict(R=R, C=C, vec=vec, mx=mx, S=S)   # noqa: E731
    assert AO.launch_tiles([t(128, 128)]) == (32, [32], 8)
    assert AO.launch_tiles([t(70, 128)], 64) == (64, [64], 4)
    assert AO.launch_tiles([t(96, 100)], 16) == (16, [16], 12)
    assert AO.launch_tiles([t(64, 64, mx=True), t(128, 64), t(33, 7, vec=False)]) == (64, [64, 32, 64], 1 + 4 + 1)
    assert AO.launch_tiles([t(64, 64, S=2), t(64, 64, S=4), t(64, 64, S=8)], 64) == (64, [64, 32, 16], 1 + 2 + 4)
    assert AO.launch_tiles([t(64, 64, S=2), t(64, 64, S=4), t(64, 64, S=8)]) == (32, [32, 16, 16], 2 + 4 + 4)


# ---------------------------------------------------------------------------- the host-device path
def _torch_adamw(p, g, m, v, h):
    """torch's own f32 evaluation: one torch.optim.AdamW step from the given moments and count."""
    tp = torch.tensor(p).requires_grad_()
    opt = torch.optim.AdamW([tp], lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd, foreach=False)
    opt.state[tp] = {"step": torch.tensor(float(h.t - 1)), "exp_avg": torch.tensor(m).clone(),
                     "exp_avg_sq": torch.tensor(v).clone()}
    tp.grad = torch.tensor(g)
    opt.step()
    st = opt.state[tp]
    return tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("name", AO.case_names())
def test_torch_path_against_oracle(name):
    """ops/optim_kernels._torch_adam (host devices, and GPU shards under a schedule's tensor lr)
    within 4 E_ref + 2^-23 max|oracle| of the float64 oracle, E_ref the error of torch.optim.AdamW
    in f32 on the same inputs."""
    from learning_jax_sharding_amd.ops.optim_kernels import _torch_adam
    h, p, g, m, v = AO.make_case(name, 4096)
    want = AO.oracle(p, g, m, v, h)
    ref = _torch_adamw(p, g, m, v, h)
    tp, tg, tm, tv = (torch.tensor(a) for a in (p, g, m, v))
    u, m2, v2 = _torch_adam(tp, tg, tm, tv, torch.tensor(h.t, dtype=torch.int32), h.lr, h.b1, h.b2, h.eps, h.wd)
    got = ((tp + u).numpy(), m2.numpy(), v2.numpy())
    for k, out in enumerate("pmv"):
        allowed = CO.host_allowed(want[k], ref[k])
        err = float(np.abs(AO.a64(got[k]) - want[k]).max())
        print(f"adam-figures host _torch_adam {name} {out} max_abs_err={err:.3e} allowed={allowed:.3e} "
              f"worst_fraction_of_bound={err / allowed:.3f}")
        assert err <= allowed, (name, out, err, allowed)


def test_adamw_apply_equals_update_plus_apply_updates(host_devices):
    """On host devices the fused ``apply`` and optax-style ``update`` + ``apply_updates`` are the same
    computation: equal bits over three steps with wd > 0, and both follow the oracle."""
    host_devices(2)
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd import optim
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh((2,)), ("data",))
    sh = NamedSharding(mesh, P("data"))
    rng = np.random.default_rng(3)
    P0 = {"w": rng.standard_normal((6, 4)).astype(np.float32), "b": rng.standard_normal((4,)).astype(np.float32)}
    put = lambda t: {"w": ljs.device_put(t["w"], sh), "b": ljs.device_put(t["b"], NamedSharding(mesh, P()))}   # noqa: E731
    tx = optim.adamw(1e-2, weight_decay=0.1)
    pa, pb = put(P0), put(P0)
    sa, sb = tx.init(pa), tx.init(pb)
    want = {k: (x, np.zeros_like(x), np.zeros_like(x)) for k, x in P0.items()}
    for step in range(3):
        G = {k: rng.standard_normal(x.shape).astype(np.float32) for k, x in P0.items()}
        pa, sa = tx.apply(pa, put(G), sa)
        upd, sb = tx.update(put(G), sb, pb)
        pb = optim.apply_updates(pb, upd)
        h = AO.Hyper(1e-2, 0.9, 0.999, 1e-8, 0.1, step + 1)
        for k in P0:
            a, b = np.asarray(pa[k]), np.asarray(pb[k])
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (step, k)
            for x, y in ((sa[0].mu[k], sb[0].mu[k]), (sa[0].nu[k], sb[0].nu[k])):
                assert np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)), (step, k)
            # the oracle runs from the path's own f32 state of the step before
            o = AO.oracle(want[k][0], G[k], want[k][1], want[k][2], h)
            ref = _torch_adamw(want[k][0], G[k], want[k][1], want[k][2], h)
            got = (a, np.asarray(sa[0].mu[k]), np.asarray(sa[0].nu[k]))
            for i, out in enumerate("pmv"):
                err = float(np.abs(AO.a64(got[i]) - o[i]).max())
                assert err <= CO.host_allowed(o[i], ref[i].reshape(-1)), (step, k, out, err)
            want[k] = tuple(np.array(x, dtype=np.float32) for x in got)
        assert int(np.asarray(sa[0].count)) == int(np.asarray(sb[0].count)) == step + 1
