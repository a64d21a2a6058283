"""``attn_extend`` (csrc/kernels/decode.hip, the EXT instances of the decode kernel) on a real MI355X.

The contract: row ``(b, t, h)`` of ``ljs_attn_extend`` / ``ljs_attn_extend_q8`` has the BITS ``ljs_attn_decode`` / ``_q8`` writes
for ``(b, h)`` with ``extra = t + 1`` under the same plan.  Checked as integers (o as int16, lse2 as int32) at B = 3,
capacities 96 and 640, a forced plan of one split and one of three splits (32-key multiples), lengths 0, 5, ``cap - T``
and ``cap - 1`` (the last clamps at the capacity), G in {1, 2, 4, 8, 16}, T in {1, 2, 3, 5, 16}; rows at and beyond ``lens
+ T`` hold NaN (bf16) or the 0x7F / 0xFF bytes and scale bytes of the formats' NaNs (MX-fp8); ``q`` is a strided column
view of a wider buffer.  Then the float64 oracle of tests/attn_oracle.py with the decode tests' bounds, bit-equal
re-runs, the launch records (``T == 1`` is ``attn_decode<..>`` itself) and the refusals."""
import pytest
import torch

import attn_oracle as AO

pytestmark = pytest.mark.gpu

SCALE = 0.125
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
B, HKV = 3, 2
CAPS = {96: [(1, 96), (3, 32)], 640: [(1, 640), (3, 224)]}
GROUPS = [1, 2, 4, 8, 16]
TS = [1, 2, 3, 5, 16]
INVALID = 1      # hipErrorInvalidValue
# the logged instance: heads per group as attn_decode names them, positions per block (8 / G, no more than T needs)
POSITIONS = {1: lambda T: 2 if T <= 2 else (4 if T <= 4 else 8), 2: lambda T: 2 if T <= 2 else 4, 4: lambda T: 2,
             8: lambda T: 1, 16: lambda T: 1}


def _hip():
    from learning_jax_sharding_amd.ops import hip
    return hip


@pytest.fixture(autouse=True)
def _default_plan():
    yield
    _hip().set_decode_splits(None)


def _lens(cap, T):
    return [[0, 5, cap - T], [cap - 1, cap - T, 5]]


def _strided_q(q):
    """``q`` (B, T, H, 64) as a column view of a wider buffer on the GPU."""
    Bq, T, H, _ = q.shape
    wide = torch.zeros(Bq, T, H * 64 + 64, dtype=BF16).cuda()
    wide[..., :H * 64] = q.cuda().view(Bq, T, H * 64)
    qv = wide[..., :H * 64].view(Bq, T, H, 64)
    assert not qv.is_contiguous()
    return qv


_DATA = {}


def _data(cap, H):
    """q for the largest T, a bf16 cache and its MX-fp8 form (CPU), made once per shape and left unchanged."""
    if (cap, H) not in _DATA:
        from learning_jax_sharding_amd.ops.kernels import _mx_bytes
        gen = torch.Generator().manual_seed(cap + H)
        q = torch.randn(B, max(TS), H, 64, generator=gen).to(BF16)
        kc = torch.randn(B, cap, HKV, 64, generator=gen).to(BF16)
        vc = torch.randn(B, cap, HKV, 64, generator=gen).to(BF16)
        _DATA[(cap, H)] = (q, kc, vc, _mx_bytes(kc), _mx_bytes(vc))
    return _DATA[(cap, H)]


def _poisoned(cap, H, lens, T):
    """(bf16 caches, MX-fp8 buffers) on the GPU with everything at and beyond ``lens + T`` poisoned."""
    _, kc, vc, (kq, ke), (vq, ve) = _data(cap, H)
    kc, vc, kq, ke, vq, ve = (t.clone() for t in (kc, vc, kq, ke, vq, ve))
    for b, n in enumerate(lens):
        kc[b, n + T:] = float("nan")
        vc[b, n + T:] = float("nan")
        kq[b, n + T:] = 0x7F
        vq[b, n + T:] = 0xFF
        ke[b, n + T:] = 0xFF
        ve[b, n + T:] = 0xFF
    return (kc.cuda(), vc.cuda()), (kq.cuda(), vq.cuda(), ke.cuda(), ve.cuda())


def _bits(o, lse):
    return o.contiguous().view(torch.int16), lse.contiguous().view(torch.int32)


def _assert_rows_are_decode(name, hip, q, lt, bf, q8):
    T = q.shape[1]
    for form, ext, dec, bufs in (("bf16", hip.attn_extend, hip.attn_decode, bf),
                                 ("mx8", hip.attn_extend_q8, hip.attn_decode_q8, q8)):
        o, lse = ext(q, *bufs, lt, SCALE)
        assert o.shape == q.shape and o.dtype == BF16 and lse.shape == (B, q.shape[2], T) and lse.dtype == F32
        assert torch.isfinite(o.float()).all(), (name, form)
        for t in range(T):
            wo, wl = dec(q[:, t:t + 1], *bufs, lt, SCALE, t + 1)
            go, gl = _bits(o[:, t:t + 1], lse[..., t:t + 1])
            eo, el = _bits(wo, wl)
            assert torch.equal(go, eo) and torch.equal(gl, el), (name, form, t)


@pytest.mark.parametrize("G", GROUPS, ids=[f"g{g}" for g in GROUPS])
@pytest.mark.parametrize("cap,plan", [(c, p) for c, ps in CAPS.items() for p in ps],
                         ids=[f"cap{c}-{p[0]}x{p[1]}" for c, ps in CAPS.items() for p in ps])
def test_extend_rows_have_decode_bits(cap, plan, G):
    hip = _hip()
    hip.set_decode_splits(*plan)
    H = G * HKV
    qfull = _data(cap, H)[0]
    for T in TS:
        q = _strided_q(qfull[:, :T])
        for lens in _lens(cap, T):
            bf, q8 = _poisoned(cap, H, lens, T)
            lt = torch.tensor(lens, dtype=torch.int32).cuda()
            _assert_rows_are_decode(f"cap{cap} plan{plan} G{G} T{T} lens{lens}", hip, q, lt, bf, q8)
    torch.cuda.synchronize()


@pytest.mark.parametrize("G", [3, 6, 12], ids=["g3", "g6", "g12"])
def test_groups_between_instances(G):
    """Group sizes that run the next larger instance with idle rows (3 -> G4, 6 -> G8, 12 -> G16)."""
    hip = _hip()
    hip.set_decode_splits(3, 32)
    cap, H, T = 96, G * HKV, 5
    q = _strided_q(_data(cap, H)[0][:, :T])
    lens = [0, 5, cap - 2]
    bf, q8 = _poisoned(cap, H, lens, T)
    _assert_rows_are_decode(f"G{G}", hip, q, torch.tensor(lens, dtype=torch.int32).cuda(), bf, q8)


@pytest.mark.parametrize("kind", AO.KINDS)
def test_extend_matches_oracle(kind):
    """The float64 oracle per (sequence, position), with the bounds of tests/test_decode_gpu.py."""
    hip = _hip()
    cap, H, T, lens = 640, 8, 3, [0, 130, 637]
    q, k, v, _ = AO.inputs(kind, B, H, T, cap, SCALE)
    k, v = k[:, :, :HKV].contiguous(), v[:, :, :HKV].contiguous()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    for plan in CAPS[cap] + [None]:
        hip.set_decode_splits(*plan) if plan else hip.set_decode_splits(None)
        o, lse = hip.attn_extend(_strided_q(q), k.cuda(), v.cuda(), lt, SCALE)
        o, lse = o.cpu(), lse.cpu()
        for b, n0 in enumerate(lens):
            for t in range(T):
                n = min(n0 + t + 1, cap)
                qb = q[b:b + 1, t:t + 1]
                kb, vb = (x[b:b + 1, :n].repeat_interleave(H // HKV, 2) for x in (k, v))
                want_o, want_lse = AO.forward(qb, kb, vb, SCALE)
                model_o, _ = AO.forward(qb, kb, vb, SCALE, rounded=True)
                name = f"extend {kind} plan{plan} b{b} t{t}"
                AO.check(f"{name} o", o[b:b + 1, t:t + 1], want_o, model_o)
                AO.check_lse(lse[b:b + 1, :, t:t + 1], want_lse, AO.lse2_f32(qb, kb, SCALE), name=f"{name} lse")


def test_launch_records_and_reruns():
    hip = _hip()
    cap = 640
    for G in GROUPS:
        H = G * HKV
        for plan in CAPS[cap]:
            hip.set_decode_splits(*plan)
            for T in TS:
                lens = [0, 5, cap - T]
                q = _strided_q(_data(cap, H)[0][:, :T])
                bf, q8 = _poisoned(cap, H, lens, T)
                lt = torch.tensor(lens, dtype=torch.int32).cuda()
                for tag, ext, bufs in (("", hip.attn_extend, bf), (",mx8", hip.attn_extend_q8, q8)):
                    with hip.launch_log() as log:
                        first = ext(q, *bufs, lt, SCALE)
                    again = ext(q, *bufs, lt, SCALE)
                    assert all(torch.equal(x, y) for x, y in zip(_bits(*first), _bits(*again))), (G, plan, T, tag)
                    merge = [{"name": "decode_merge", "grid": (B * T * H, 1, 1)}] if plan[0] > 1 else []
                    if T == 1:       # a one-position call IS attn_decode: its launches, its records
                        want = [{"name": f"attn_decode<G{G}{tag}>", "grid": (plan[0], HKV, B)}]
                    else:
                        P = POSITIONS[G](T)
                        want = [{"name": f"attn_extend<G{G},P{P}{tag}>", "grid": (plan[0] * -(-T // P), HKV, B)}]
                    got = [{"name": r["name"], "grid": tuple(r["grid"])} for r in log]
                    assert got == want + merge, (got, want + merge)
                    assert log[0]["block"] == 256
    torch.cuda.synchronize()


def test_default_plan_and_dispatch():
    """The plan function's own plan at cap = 1024 (more than one split) through ``ops.kernels``."""
    from learning_jax_sharding_amd.ops import kernels as K
    hip = _hip()
    cap, H, T, lens = 1024, 8, 4, [1000, 3, 600]
    gen = torch.Generator().manual_seed(9)
    q = torch.randn(B, T, H, 64, generator=gen).to(BF16).cuda()
    kc = torch.randn(B, cap, HKV, 64, generator=gen).to(BF16).cuda()
    vc = torch.randn(B, cap, HKV, 64, generator=gen).to(BF16).cuda()
    lt = torch.tensor(lens, dtype=torch.int32).cuda()
    splits, _ = hip.plan_decode(B, HKV, cap)
    assert splits > 1
    with hip.launch_log() as log:
        o, lse = K.attn_extend(q, kc, vc, lt, SCALE)
    assert [r["name"] for r in log] == ["attn_extend<G4,P2>", "decode_merge"] and log[0]["grid"] == (splits * 2, HKV, B), log
    for t in range(T):
        wo, wl = K.attn_decode(q[:, t:t + 1], kc, vc, lt, SCALE, extra=t + 1)
        assert torch.equal(o[:, t:t + 1], wo) and torch.equal(lse[..., t:t + 1], wl), t
    d = torch.tensor([2, -3, 0], dtype=torch.int32).cuda()
    assert K.lens_add_delta(lt, d) is lt and lt.tolist() == [1002, 0, 600]


def test_bad_arguments_launch_nothing():
    hip = _hip()
    assert hip.extend_max_positions() == 64
    kc = torch.zeros(2, 64, 2, 64, dtype=BF16).cuda()
    k8 = torch.zeros(2, 64, 2, 64, dtype=U8).cuda()
    ks = torch.zeros(2, 64, 2, 2, dtype=U8).cuda()
    lens = torch.zeros(2, dtype=torch.int32).cuda()
    ws = torch.empty(1 << 20).cuda()

    def ops(T, H=8):
        q = torch.zeros(2, T, H, 64, dtype=BF16).cuda()
        return q, torch.empty_like(q), torch.empty(2, T, H).cuda()

    n0 = hip.lib().ljs_launch_count()
    q, o, lse = ops(4)
    assert hip.attn_extend_raw(q, kc, kc, o, lse, ws, lens, SCALE) == 0                      # (the good calls)
    assert hip.attn_extend_q8_raw(q, k8, k8, ks, ks, o, lse, ws, lens, SCALE) == 0
    n1 = hip.lib().ljs_launch_count()
    assert n1 == n0 + 2
    q65, o65, lse65 = ops(65)
    assert hip.attn_extend_raw(q65, kc, kc, o65, lse65, ws, lens, SCALE) == INVALID          # T > 64
    assert hip.attn_extend_q8_raw(q65, k8, k8, ks, ks, o65, lse65, ws, lens, SCALE) == INVALID
    q32, o32, lse32 = ops(4, 64)
    assert hip.attn_extend_raw(q32, kc, kc, o32, lse32, ws, lens, SCALE) == INVALID          # G = 32
    assert hip.attn_extend_raw(q, kc, kc, o, lse, ws, lens, 0.0) == INVALID                  # scale <= 0
    hip.set_decode_splits(2, 32)
    assert hip.attn_extend_raw(q, kc, kc, o, lse, None, lens, SCALE) == INVALID              # no workspace for 2 splits
    assert hip.attn_extend_raw(q, kc, kc, o, lse, ws[:1024], lens, SCALE) == INVALID         # too small for B T H
    hip.set_decode_splits(None)
    assert hip.lib().ljs_launch_count() == n1
    with pytest.raises(NotImplementedError, match="attn_extend"):
        hip.attn_extend(q65, kc, kc, lens, SCALE)
    torch.cuda.synchronize()
