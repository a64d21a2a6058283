"""Sampling on host devices: ``sample_reference`` against the float64 oracle of tests/sample_oracle.py, the
distribution of its draws, the properties of its random stream, ``random.categorical`` and ``generate`` with a
key and with stop tokens."""
import numpy as np
import pytest
import torch

import sample_oracle as SO
from test_decode import LM, PLENS, lm_params, mesh_setup, tokens

BF16, F32 = torch.bfloat16, torch.float32
T = 0.7
CHI2_15_9999 = 44.263      # the 99.99 % quantile of chi-square with 15 degrees of freedom
CHI2_3_9999 = 21.108       # ... with 3 (a support of four)
CHI2_2_9999 = 18.421       # ... with 2 (a support of three)


def _key(seed=7):
    import learning_jax_sharding_amd as ljs
    return ljs.random.PRNGKey(seed)


def check_against_oracle(name, x, got, key, batch_offset=0, pos=None, pmargin=1e-3, **kw):
    """``got = (tokens, kept, tau)`` of ``[B, V]`` logits ``x`` (a float tensor) against the oracle: kept and tau exact
    (on rows the oracle holds >= 1e-3 away from p, asserted), tokens equal wherever the oracle's gap exceeds the
    margin.  Returns the number of rows left out."""
    tok, kept, tau = (t.cpu() for t in got)
    want = SO.sample(x.double().cpu().numpy(), key, batch_offset, None if pos is None else pos.cpu().numpy(), **kw)
    left_out = 0
    for b, w in enumerate(want):
        assert w["pmargin"] >= pmargin, (name, b, w["pmargin"])          # the precondition, on the oracle alone
        assert int(kept[b]) == w["kept"], (name, b, int(kept[b]), w["kept"])
        assert float(tau[b]) == w["tau"], (name, b, float(tau[b]), w["tau"])
        if w["gap"] > SO.margin(w["score"]):
            assert int(tok[b]) == w["token"], (name, b, int(tok[b]), w)
        else:
            left_out += 1
    return left_out


# ----------------------------------------------------------------------------- 1. the reference
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [8, 1001, 4104])
def test_reference_matches_oracle(V, B, dtype):
    from learning_jax_sharding_amd.ops import kernels as K
    x = torch.from_numpy(SO.rows(B, V, T, seed=V + B, bf16=dtype == BF16)).to(dtype)
    pos = torch.arange(B, dtype=torch.int32) * 3 + 11
    key = _key()
    for name, kw in SO.modes(V, T):
        tok = torch.empty(B, dtype=torch.int64)
        got = K.sample_reference(x, tok, key, pos=pos, batch_offset=5, stats=True, **kw)
        assert got[0] is tok
        assert check_against_oracle(f"{name} V{V} B{B}", x, got, key, 5, pos, **kw) == 0, name
    got = K.sample_reference(x, torch.empty(B, dtype=torch.int64), key, pos=pos, top_p=SO.P_TINY, stats=True)
    assert got[1].tolist() == [1] * B
    assert check_against_oracle(f"p tiny V{V} B{B}", x, got, key, 0, pos, pmargin=SO.P_TINY, top_p=SO.P_TINY) == 0
    none = K.sample_reference(x, torch.empty(B, dtype=torch.int64), key, pos=pos, temperature=T).clone()
    for kw in (dict(top_k=V), dict(top_k=V + 7), dict(top_p=1.0)):          # no filter at all
        tok, kept, _ = K.sample_reference(x, torch.empty(B, dtype=torch.int64), key, pos=pos, temperature=T,
                                          stats=True, **kw)
        assert torch.equal(tok, none) and kept.tolist() == [V] * B, kw
    # top_k = 1 (no tie at the maximum here) is the greedy argmax, which needs no key
    greedy = K.sample_reference(x, torch.empty(B, dtype=torch.int32))
    assert greedy.dtype == torch.int32 and torch.equal(greedy.long(), x.float().argmax(-1))
    one = K.sample_reference(x, torch.empty(B, dtype=torch.int64), key, pos=pos, top_k=1)
    assert torch.equal(one, greedy.long())


def test_reference_edges():
    from learning_jax_sharding_amd.ops import kernels as K
    key = _key()
    V = 1001
    # a tied maximum: a tiny top_p keeps exactly its tie group, top_k = 1 both of its entries
    x = torch.from_numpy(SO.rows(3, V, seed=3, head=(2, 2, 2)))
    for kw in (dict(top_p=SO.P_TINY), dict(top_k=1)):
        got = K.sample_reference(x, torch.empty(3, dtype=torch.int64), key, stats=True, **kw)
        assert got[1].tolist() == [2, 2, 2] and torch.equal(got[2], x.amax(-1)), kw
        assert check_against_oracle(f"tied max {kw}", x, got, key, pmargin=SO.P_TINY, **kw) == 0
        assert all(x[b, got[0][b]] == x[b].max() for b in range(3))
    # greedy: the lowest index of a tied maximum
    first = [int((x[b] == x[b].max()).nonzero()[0]) for b in range(3)]
    assert K.sample_reference(x, torch.empty(3, dtype=torch.int64)).tolist() == first
    # tied logits straddling the k-th place are all kept: HEAD = (1, 1, 2), k = 3 keeps 4
    x = torch.from_numpy(SO.rows(3, V, seed=4))
    assert K.sample_reference(x, torch.empty(3, dtype=torch.int64), key, top_k=3, stats=True)[1].tolist() == [4] * 3
    # -inf entries are never drawn, with and without filters, and count as the oracle counts them
    x[:, ::2] = float("-inf")
    x[1, 1::2] = float("-inf")
    x[1, 500] = 0.25                                     # one finite entry left
    for kw in (dict(), dict(top_k=600), dict(top_p=0.5), dict(top_k=40, top_p=0.5)):
        for p in range(20):
            pos = torch.full((3,), p, dtype=torch.int64)
            tok, kept, tau = K.sample_reference(x, torch.empty(3, dtype=torch.int64), key, pos=pos, stats=True, **kw)
            assert torch.isfinite(x[torch.arange(3), tok]).all() and int(tok[1]) == 500, (kw, p)
        want = SO.sample(x.double().numpy(), key, pos=pos.numpy(), **kw)
        assert kept.tolist() == [w["kept"] for w in want] and tau.tolist() == [w["tau"] for w in want], kw
    # outside the contract, an index of the row all the same
    bad = torch.full((2, 16), float("-inf"))
    bad[1] = float("nan")
    for k in (None, key):
        tok = K.sample_reference(bad, torch.empty(2, dtype=torch.int64), k)
        assert ((tok >= 0) & (tok < 16)).all()
    # [B, T, V] logits: the row at[b], clamped; default the last
    x3 = torch.randn(3, 4, 64, generator=torch.Generator().manual_seed(0))
    at = torch.tensor([0, 2, 9])
    got = K.sample_reference(x3, torch.empty(3, 1, dtype=torch.int64), key, at=at)
    want = K.sample_reference(torch.stack([x3[0, 0], x3[1, 2], x3[2, 3]]), torch.empty(3, dtype=torch.int64), key)
    assert got.shape == (3, 1) and torch.equal(got.reshape(3), want)
    last = K.sample_reference(x3, torch.empty(3, dtype=torch.int64), key)
    assert torch.equal(last, K.sample_reference(x3[:, -1], torch.empty(3, dtype=torch.int64), key))


def test_reference_stop_tokens():
    from learning_jax_sharding_amd.ops import kernels as K
    x = torch.full((4, 16), -5.0)
    x[0, 3] = x[1, 9] = x[2, 4] = x[3, 3] = 5.0          # the argmax of each row
    done = torch.tensor([0, 0, 0, 1], dtype=torch.int32)
    tok = K.sample_reference(x, torch.empty(4, dtype=torch.int64), done=done, eos=(3, 9), pad=15)
    assert tok.tolist() == [3, 9, 4, 15] and done.tolist() == [1, 1, 0, 1]
    tok = K.sample_reference(x, torch.empty(4, dtype=torch.int64), done=done, eos=(3, 9), pad=15)
    assert tok.tolist() == [15, 15, 4, 15] and done.tolist() == [1, 1, 0, 1]


# ----------------------------------------------------------------------------- 2. the distribution
def _draws(x, key, n, **kw):
    from learning_jax_sharding_amd.ops import kernels as K
    rows = x[None, :].expand(n, -1)
    pos = torch.arange(n, dtype=torch.int64)
    return K.sample_reference(rows, torch.empty(n, dtype=torch.int64), key, pos=pos, **kw).numpy()


def chi_square(tokens, probs):
    n = len(tokens)
    counts = np.bincount(tokens, minlength=len(probs)).astype(np.float64)
    assert counts[probs == 0].sum() == 0, "a draw outside the support"
    live = probs > 0
    return float((((counts - n * probs) ** 2)[live] / (n * probs[live])).sum())


DIST_X = torch.tensor([1.5, -0.3, 0.9, 2.2, -1.0, 0.1, 1.1, -2.0, 0.4, 1.9, -0.6, 0.7, 2.6, -1.4, 0.0, 1.3])


def test_distribution_matches_softmax():
    """20000 draws at V = 16 by varying pos, one fixed key (so nothing here is random from run to run): chi-square
    against the exact softmax below the 99.99 % quantile, for the whole row and for the renormalised top-k = 4 and
    top-p = 0.7 supports, with no draw outside a support."""
    key, n = _key(2024), 20000
    p = torch.softmax(DIST_X.double() / T, -1).numpy()
    assert chi_square(_draws(DIST_X, key, n, temperature=T), p) < CHI2_15_9999
    top4 = np.where(p >= np.sort(p)[-4], p, 0.0)
    assert chi_square(_draws(DIST_X, key, n, temperature=T, top_k=4), top4 / top4.sum()) < CHI2_3_9999
    mask, _, pmargin = SO.kept_set(DIST_X.numpy(), T, None, 0.7)
    assert pmargin >= 1e-3 and 1 < mask.sum() < 16
    nucleus = np.where(mask, p, 0.0)
    stat = chi_square(_draws(DIST_X, key, n, temperature=T, top_p=0.7), nucleus / nucleus.sum())
    assert mask.sum() == 3 and stat < CHI2_2_9999, (mask.sum(), stat)


# ----------------------------------------------------------------------------- 3. the stream
def test_stream_properties():
    from learning_jax_sharding_amd.ops import kernels as K
    B, V = 8, 1001
    x = torch.randn(B, V, generator=torch.Generator().manual_seed(1)) * 0.1      # flat: the noise decides
    pos = torch.arange(B, dtype=torch.int32) + 40
    draw = lambda key=_key(), x=x, **kw: K.sample_reference(x, torch.empty(x.shape[0], dtype=torch.int64), key,  # noqa: E731
                                                            **kw)
    base = draw(pos=pos, batch_offset=16)
    assert torch.equal(base, draw(pos=pos, batch_offset=16))
    for other in (draw(pos=pos + 1, batch_offset=16), draw(pos=pos, batch_offset=17), draw(_key(8), pos=pos,
                                                                                          batch_offset=16)):
        assert (other != base).sum() >= B - 1
    # global row b alone with batch_offset = b, and inside a batch
    for b in range(B):
        alone = draw(x=x[b:b + 1], pos=pos[b:b + 1], batch_offset=16 + b)
        assert int(alone[0]) == int(base[b]), b


# ----------------------------------------------------------------------------- 4. random.categorical
def test_categorical(host_devices):
    import learning_jax_sharding_amd as ljs
    from learning_jax_sharding_amd.ops import kernels as K
    host_devices(1)
    key = _key(5)
    x = torch.randn(3, 5, 33, generator=torch.Generator().manual_seed(2))
    got = ljs.random.categorical(key, ljs.device_put(x.numpy()))
    assert got.shape == (3, 5) and got.dtype == torch.int32
    want = K.sample_reference(x.reshape(15, 33), torch.empty(15, dtype=torch.int32), key)      # hi = row, lo = 0
    assert torch.equal(got.to_torch().reshape(-1), want)
    ax = ljs.random.categorical(key, ljs.device_put(x.movedim(-1, 1).contiguous().numpy()), axis=1)
    assert torch.equal(ax.to_torch(), got.to_torch())
    many = ljs.random.categorical(key, ljs.device_put(DIST_X.numpy()), shape=(20000,))
    assert many.shape == (20000,)
    assert chi_square(many.to_torch().numpy(), torch.softmax(DIST_X.double(), -1).numpy()) < CHI2_15_9999
    with pytest.raises(ValueError, match="broadcast"):
        ljs.random.categorical(key, ljs.device_put(x.numpy()), shape=(4, 5))
    host_devices(2)
    from learning_jax_sharding_amd.mesh import Mesh, create_device_mesh
    from learning_jax_sharding_amd.sharding import NamedSharding, PartitionSpec as P
    mesh = Mesh(create_device_mesh((2,)), ("data",))
    x4 = torch.randn(4, 5, 34, generator=torch.Generator().manual_seed(3))
    host = K.sample_reference(x4.reshape(20, 34), torch.empty(20, dtype=torch.int32), key).reshape(4, 5)
    for spec in (P("data"), P(None, None, "data")):
        two = ljs.random.categorical(key, ljs.device_put(x4.numpy(), NamedSharding(mesh, spec)))
        assert torch.equal(two.to_torch(), host), spec


# ----------------------------------------------------------------------------- 5. generate
def _setup(host_devices, seed=8):
    from learning_jax_sharding_amd.models import TransformerLM
    host_devices(1)
    tok = tokens(seed=seed)
    params, put = lm_params(LM, tok)
    return TransformerLM(**LM, dtype=F32), params, put(tok[:, :max(PLENS)].numpy()), tok, put


def test_generate_sampling(host_devices):
    from learning_jax_sharding_amd.models import generate
    model, params, ids, tok, put = _setup(host_devices)
    greedy = generate(model, params, ids, 8, prompt_lens=PLENS)
    assert greedy.shape == (4, 8) and greedy.dtype == torch.int64
    key = _key(1)
    a = generate(model, params, ids, 8, prompt_lens=PLENS, key=key, temperature=50.0)
    b = generate(model, params, ids, 8, prompt_lens=PLENS, key=key, temperature=50.0)
    c = generate(model, params, ids, 8, prompt_lens=PLENS, key=_key(2), temperature=50.0)
    assert a.shape == (4, 8) and torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, greedy)
    # a vanishing temperature and top_k = 1 are both the argmax
    for kw in (dict(temperature=1e-4), dict(top_k=1)):
        assert torch.equal(generate(model, params, ids, 8, prompt_lens=PLENS, key=key, **kw), greedy), kw
    toks, lens = generate(model, params, ids, 8, prompt_lens=PLENS, return_lens=True)
    assert torch.equal(toks, greedy) and lens.tolist() == [8] * 4


def test_generate_stop_tokens(host_devices):
    """Greedy with stop tokens: the eos ids are tokens the greedy run is known to produce, at known steps."""
    from learning_jax_sharding_amd.models import generate
    model, params, ids, tok, put = _setup(host_devices)
    greedy = generate(model, params, ids, 8, prompt_lens=PLENS)
    eos = [int(greedy[0, 2]), int(greedy[1, 0])]
    pad = 256
    want, want_lens = greedy.clone(), []
    for b in range(4):
        hit = [s for s in range(8) if int(greedy[b, s]) in eos]
        n = hit[0] + 1 if hit else 8
        want[b, n:] = pad
        want_lens.append(n)
    assert want_lens[0] <= 3 and want_lens[1] == 1
    for poll in (16, 1, 0):
        got, lens = generate(model, params, ids, 8, prompt_lens=PLENS, eos_id=eos, pad_id=pad, stop_poll=poll,
                             return_lens=True)
        assert got.shape == (4, 8) and torch.equal(got, want) and lens.tolist() == want_lens, poll
    # every sequence stops at once: the early exit still returns [B, max_new_tokens]
    first = sorted(set(greedy[:, 0].tolist()))
    got, lens = generate(model, params, ids, 8, prompt_lens=PLENS, eos_id=first, pad_id=pad, stop_poll=1,
                         return_lens=True)
    assert got.shape == (4, 8) and torch.equal(got[:, 0], greedy[:, 0]) and (got[:, 1:] == pad).all()
    assert lens.tolist() == [1] * 4
    one = generate(model, params, ids, 8, prompt_lens=PLENS, eos_id=int(greedy[1, 0]), pad_id=pad)
    assert torch.equal(one[1], want[1])


def test_generate_errors(host_devices):
    from learning_jax_sharding_amd.models import generate
    model, params, ids, tok, put = _setup(host_devices)
    key = _key()
    bad = [dict(key=key, temperature=0.0), dict(key=key, temperature=-1.0), dict(key=key, top_k=0),
           dict(key=key, top_p=0.0), dict(key=key, top_p=1.5), dict(top_k=5), dict(top_p=0.9), dict(eos_id=3),
           dict(eos_id=257, pad_id=0), dict(eos_id=3, pad_id=-1), dict(eos_id=3, pad_id=257),
           dict(eos_id=list(range(9)), pad_id=0), dict(eos_id=[], pad_id=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            generate(model, params, ids, 4, prompt_lens=PLENS, **kw)


def test_generate_two_devices_match_one(host_devices):
    from learning_jax_sharding_amd.models import TransformerLM, generate
    lm = dict(LM, vocab_size=256)
    tok = tokens(vocab=256, seed=8)
    host_devices(1)
    params1, put1 = lm_params(lm, tok)
    key = _key(3)
    kw = dict(prompt_lens=PLENS, key=key, temperature=20.0, top_k=50, top_p=0.95, eos_id=[7, 9], pad_id=0,
              return_lens=True)
    want = generate(TransformerLM(**lm, dtype=F32), params1, put1(tok[:, :max(PLENS)].numpy()), 6, **kw)
    for mesh_shape in ((2, 1), (1, 2)):
        host_devices(2)
        params, put, cache_sh, Ctx = mesh_setup(mesh_shape, lm, tok)
        with Ctx():
            got = generate(TransformerLM(**lm, dtype=F32), params, put(tok[:, :max(PLENS)].numpy()), 6,
                           cache_sharding=cache_sh, **kw)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), mesh_shape
