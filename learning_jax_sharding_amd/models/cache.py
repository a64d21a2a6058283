"""The key/value cache of a decoder and generation (greedy, sampled with stop tokens, or greedy with a draft model:
speculative decoding) on top of it.

A :class:`KVCache` holds, per layer, ``k`` and ``v`` of shape ``(batch, max_len, kv_heads, dim_head)`` in the
model's compute dtype (zero-filled) and ONE shared ``lens``: int32 ``(batch,)``, the rows of every
sequence that are valid.  ``lens`` lives on the devices and nowhere else: a decode step reads it
there (the position of the new token, the key count), so the step's signature and launches are the
same at every length and it can be captured once and replayed as a HIP graph.  It is a pytree
(``jit`` and ``tree_util`` flatten it); the buffers are updated in place and a cached call returns the
same buffers (donation semantics).

Layout: like ``k`` after the head split with the length dim whole.  A cache sharded on its batch dim
(data parallel) or on its ``kv_heads`` dim (tensor parallel, ``kv_heads % n == 0``) needs no collective;
a length-sharded cache raises ``NotImplementedError``.

``quant="mxfp8"`` (opt-in) makes the cache MX-fp8: ``k`` / ``v`` hold OCP e4m3 bytes (uint8, the same shape) and
``k_scale`` / ``v_scale`` one e8m0 byte per 32 elements of a head row (uint8 ``(batch, max_len, kv_heads, dim_head /
32)``), laid out and sharded like the buffers: 66 bytes per cached head row of 64 instead of 128.  An appended row
is ``ops.fp8.quantize_mx_ref`` of the row the unquantised cache would hold, and a decode step attends to the
dequantised rows (``ops.kernels.kv_append_q8_reference`` / ``attn_decode_q8_reference`` state both).  A prefill attends
to the prompt's own unquantised K / V and then stores them quantised, so the first generated token has seen
bf16 keys and the later ones see fp8 keys.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import dtypes as _dt
from ..array import ShardedArray, device_put
from ..ops import core
from ..ops import kernels as K
from ..runtime.devices import get_device, process_index
from ..sharding.shardings import Sharding, default_sharding, sharding_from_tile
from ..utils import tree as _tree

__all__ = ["KVCache", "generate"]

QUANT_MXFP8 = "mxfp8"


class KVCache:
    """``k[i]``, ``v[i]``: layer i's buffers; ``lens``: the shared int32 ``(batch,)`` lengths; ``k_scale[i]``, ``v_scale[i]``:
    layer i's e8m0 scales in an MX-fp8 cache (empty lists without ``quant``)."""

    def __init__(self, k: Sequence[ShardedArray], v: Sequence[ShardedArray], lens: ShardedArray,
                 k_scale: Sequence[ShardedArray] = (), v_scale: Sequence[ShardedArray] = ()):
        self.k, self.v, self.lens = list(k), list(v), lens
        self.k_scale, self.v_scale = list(k_scale), list(v_scale)
        if len(self.k_scale) != len(self.v_scale) or len(self.k_scale) not in (0, len(self.k)):
            raise ValueError(f"KVCache: {len(self.k_scale)} / {len(self.v_scale)} scale buffers for {len(self.k)} layers")

    @property
    def quant(self) -> Optional[str]:
        return QUANT_MXFP8 if self.k_scale else None

    def layer(self, i: int):
        """``(k, v, lens)`` of layer ``i``, or ``(k, v, lens, k_scale, v_scale)`` of a quantised cache: what
        ``MultiHeadAttention(..., cache=)`` takes."""
        if self.k_scale:
            return self.k[i], self.v[i], self.lens, self.k_scale[i], self.v_scale[i]
        return self.k[i], self.v[i], self.lens

    @property
    def nbytes(self) -> int:
        """Bytes of the k / v buffers and their scales (all devices, without ``lens``)."""
        return sum(int(np.prod(a.shape)) * a.dtype.itemsize for a in self.k + self.v + self.k_scale + self.v_scale)

    @property
    def max_len(self) -> int:
        return self.k[0].shape[1]

    @property
    def batch(self) -> int:
        return self.k[0].shape[0]

    def __len__(self):
        return len(self.k)

    def __repr__(self):
        q = f", quant={self.quant!r}" if self.k_scale else ""
        return f"KVCache(layers={len(self.k)}, shape={self.k[0].shape if self.k else None}{q})"

    @staticmethod
    def zeros(layers: int, batch: int, max_len: int, kv_heads: int, dim_head: int, dtype=torch.bfloat16,
              sharding: Optional[Sharding] = None, quant: Optional[str] = None) -> "KVCache":
        """A zero-filled cache; ``sharding``: of the 4-D buffers (default: where unplaced arrays live); ``quant``:
        None, or ``"mxfp8"`` for uint8 e4m3 buffers with e8m0 scales (module docstring; ``dim_head % 32 == 0``,
        ``dtype`` is then the model's, not the buffers')."""
        if min(layers, batch, max_len, kv_heads, dim_head) < 1:
            raise ValueError(f"KVCache: layers={layers}, batch={batch}, max_len={max_len}, kv_heads={kv_heads}, "
                             f"dim_head={dim_head} must all be positive")
        if quant not in (None, QUANT_MXFP8):
            raise ValueError(f"KVCache: quant must be None or {QUANT_MXFP8!r}, got {quant!r}")
        if quant and dim_head % 32 != 0:
            raise ValueError(f"KVCache: quant={quant!r} needs dim_head % 32 == 0 (one scale per 32 elements), got "
                             f"{dim_head}")
        sharding = sharding or default_sharding()
        dtype = _dt.canonicalize(dtype)
        shape = (batch, max_len, kv_heads, dim_head)
        ta = sharding.tile_assignment(4)
        ta.check_shape(shape)
        if ta.tile_shape[1] > 1:
            raise NotImplementedError("KVCache: a length-sharded cache is not implemented (ring decode); shard it "
                                      "on its batch and / or kv_heads dims")
        pi = process_index()
        devs = [d for d in ta.device_ids if get_device(d).process_index == pi]

        def zeros(shp, tile, dt, sh):
            ss = tile.shard_shape(shp)
            return ShardedArray(shp, dt, sh, {d: torch.zeros(ss, dtype=dt, device=get_device(d).torch_device)
                                              for d in devs})

        lt = ta.project([0])
        lens = zeros((batch,), lt, torch.int32, sharding_from_tile(lt, like=[sharding]))
        if quant:
            ss = (batch, max_len, kv_heads, dim_head // 32)
            ta.check_shape(ss)
            u8 = lambda shp: [zeros(shp, ta, torch.uint8, sharding) for _ in range(layers)]   # noqa: E731
            return KVCache(u8(shape), u8(shape), lens, u8(ss), u8(ss))
        return KVCache([zeros(shape, ta, dtype, sharding) for _ in range(layers)],
                       [zeros(shape, ta, dtype, sharding) for _ in range(layers)], lens)


# the leaves of an unquantised cache are (k, v, lens) as ever; a quantised one adds its scales
_tree.register_pytree_node(
    KVCache, lambda c: ((c.k, c.v, c.lens, c.k_scale, c.v_scale) if c.k_scale else (c.k, c.v, c.lens), None),
    lambda _, ch: KVCache(*ch))


def _host_lens(prompt_lens, B: int, T: int) -> List[int]:
    if prompt_lens is None:
        return [T] * B
    if isinstance(prompt_lens, ShardedArray):
        prompt_lens = prompt_lens.to_torch()
    vals = [int(x) for x in np.asarray(prompt_lens).reshape(-1)]
    if len(vals) != B or any(n < 1 or n > T for n in vals):
        raise ValueError(f"generate: prompt_lens must be {B} ints in [1, {T}], got {vals}")
    return vals


def _greedy(logits: ShardedArray, like: ShardedArray, at: Optional[ShardedArray] = None) -> ShardedArray:
    """``argmax`` over the vocabulary of ``logits`` (batch, T, vocab) at position ``at[b]`` (an int (batch,) array
    laid out like the batch dim; default: the last), on the devices: ``(batch, 1)`` in ``like``'s dtype."""
    tile = logits.tile.unshard([1, 2])
    if logits.tile != tile:
        from ..spmd.reshard import reshard_tile
        logits = reshard_tile(logits, tile, note="generate.logits")
    loc = {}
    for d, t in logits.local.items():
        if at is None:
            row = t[:, -1]
        else:
            idx = at.local[d].long().clamp(0, t.shape[1] - 1)
            row = t[torch.arange(t.shape[0], device=t.device), idx]
        loc[d] = row.float().argmax(-1, keepdim=True).to(like.dtype)
    ot = tile.project([0, 1])
    return ShardedArray((logits.shape[0], 1), like.dtype, sharding_from_tile(ot, like=[logits.sharding]), loc)


def _greedy_all(logits: ShardedArray, like: ShardedArray) -> ShardedArray:
    """``argmax`` over the vocabulary at every position of ``logits`` (batch, T, vocab), on the devices: ``(batch, T)`` in
    ``like``'s dtype."""
    tile = logits.tile.unshard([1, 2])
    if logits.tile != tile:
        from ..spmd.reshard import reshard_tile
        logits = reshard_tile(logits, tile, note="generate.logits")
    loc = {d: t.float().argmax(-1).to(like.dtype) for d, t in logits.local.items()}
    return ShardedArray(tuple(logits.shape[:2]), like.dtype, sharding_from_tile(tile.project([0, 1]), like=[logits.sharding]),
                        loc)


def _draft_request(model, draft, draft_tokens, key, eos_id):
    """The checks of ``generate``'s ``draft`` arguments, on the host before any launch: ``(draft_model, draft_params, k)``."""
    from ..ops.kernels import EXTEND_MAX_POSITIONS
    if key is not None or eos_id is not None:
        raise ValueError("generate: draft= is greedy speculative decoding; it takes neither a key (sampling) nor an eos_id")
    if not isinstance(draft, (tuple, list)) or len(draft) != 2:
        raise ValueError("generate: draft must be (draft_model, draft_params)")
    k = int(draft_tokens)
    if k < 1 or k + 1 > EXTEND_MAX_POSITIONS:
        raise ValueError(f"generate: draft_tokens must be in [1, {EXTEND_MAX_POSITIONS - 1}] (the target checks draft_tokens + "
                         f"1 positions in one call), got {draft_tokens}")
    if draft[0].vocab_size != model.vocab_size:
        raise ValueError(f"generate: the draft's vocabulary ({draft[0].vocab_size}) differs from the model's "
                         f"({model.vocab_size})")
    return draft[0], draft[1], k


def _generate_speculative(model, params, draft, dparams, k: int, ids, plens, max_new_tokens: int, cache, dcache, pl,
                          capture, stop_poll: int):
    """Greedy speculative decoding (``generate``'s ``draft=``): ``(tokens [batch, max_new_tokens], mean tokens per round)``.

    One round, captured once, no host read inside.  State per sequence: ``pair``, the last two tokens of the sequence
    (the second is not in either cache yet); the target's ``lens`` counts everything before it, the draft's one less.
    The draft takes ``pair`` as one ``extend`` call (it rewrites the row of the first token with the same values, which
    makes the scheme the same whatever the last round accepted) and then ``k - 1`` single steps: ``d_1 .. d_k``.  The target
    takes ``[pair[1], d_1 .. d_k]`` as one ``extend`` call: ``g_0 .. g_k``, what it would have decoded after each.  ``a`` leading
    agreements ``d_(i+1) == g_i`` are accepted and the round emits ``g_0 .. g_a`` (``d_1 .. d_a`` and the target's own next
    token), cut so that no sequence gets more than ``max_new_tokens``; both ``lens`` are set back by ``k - a`` on the
    devices (the rows beyond are dead).  A sequence that has all its tokens emits none and stays where it is."""
    from ..spmd.api import jit
    B = ids.shape[0]
    lens = cache.lens

    def prefill(p, dp, x, c, dc, n):
        logits, c = model.apply({"params": p}, x, cache=c, prompt_lens=n)
        _, dc = draft.apply({"params": dp}, x, cache=dc, prompt_lens=n)
        core.cache_advance(dc.lens, -1)
        last = ShardedArray(n.shape, n.dtype, n.sharding, {d: t - 1 for d, t in n.local.items()})
        return _greedy(logits, x, last), c, dc

    def rnd(p, dp, st, c, dc):
        pair, toks, cnt, n_out = st
        lg, dc = draft.apply({"params": dp}, pair, cache=dc, extend=True)
        d = [_greedy(lg, pair)]
        for _ in range(k - 1):
            lg, dc = draft.apply({"params": dp}, d[-1], cache=dc)
            d.append(_greedy(lg, pair))
        x = ShardedArray((B, k + 1), pair.dtype, pair.sharding,
                         {dev: torch.cat([t[:, 1:2]] + [di.local[dev] for di in d], dim=1)
                          for dev, t in pair.local.items()})
        lg, c = model.apply({"params": p}, x, cache=c, extend=True)
        g = _greedy_all(lg, pair)
        back = {}
        for dev, gl in g.local.items():
            xl, pr, no = x.local[dev], pair.local[dev], n_out.local[dev]
            a = (xl[:, 1:] == gl[:, :k]).to(torch.int32).cumprod(1).sum(1).to(torch.int32)
            a = torch.minimum(a, max_new_tokens - 1 - no)          # -1: the sequence has all its tokens
            at = a.clamp(min=0).long()[:, None]
            new = torch.cat([xl.gather(1, at), gl.gather(1, at)], dim=1)
            pr.copy_(torch.where(a[:, None] >= 0, new, pr))
            toks.local[dev].copy_(gl)
            cnt.local[dev].copy_(a + 1)
            no.add_(a + 1)
            back[dev] = a - k
        for ln in (c.lens, dc.lens):       # both were advanced by k + 1
            core.cache_advance(ln, ShardedArray(ln.shape, ln.dtype, ln.sharding, {dev: back[dev] for dev in ln.local}))
        return st, c, dc

    rnd_j = jit(rnd, donate_argnums=(2, 3, 4), capture=capture)
    with torch.no_grad():
        tok, cache, dcache = prefill(params, dparams, ids, cache, dcache, pl)
        first = tok.to_torch().reshape(B, 1).long()
        if max_new_tokens == 1:
            return first, 0.0
        host_ids = ids.to_torch()
        prev = torch.stack([host_ids[b, n - 1] for b, n in enumerate(plens)]).reshape(B, 1)
        pair = device_put(torch.cat([prev.long(), first], dim=1).to(tok.dtype).numpy(), tok.sharding)
        zeros = lambda shape, dt, sh, like: ShardedArray(   # noqa: E731
            shape, dt, sh, {d: torch.zeros((t.shape[0],) + tuple(shape[1:]), dtype=dt, device=t.device)
                            for d, t in like.local.items()})
        toks = zeros((B, k + 1), tok.dtype, tok.sharding, tok)
        cnt = zeros((B,), torch.int32, lens.sharding, lens)
        n_out = zeros((B,), torch.int32, lens.sharding, lens)
        for t in n_out.local.values():
            t.fill_(1)                     # the prefill's token
        st = (pair, toks, cnt, n_out)
        kept = []
        for r in range(1, max_new_tokens):             # a round gives every unfinished sequence at least one token
            st, cache, dcache = rnd_j(params, dparams, st, cache, dcache)
            kept.append(({d: t.clone() for d, t in st[1].local.items()}, {d: t.clone() for d, t in st[2].local.items()}))
            # outside the graph: one host read of the counts every stop_poll rounds
            if stop_poll and r % int(stop_poll) == 0 and all(
                    bool((t >= max_new_tokens).all()) for t in st[3].local.values()):
                break
        rows = [[first[b]] for b in range(B)]
        emitted = rounds = 0
        for tl, cl in kept:
            th = ShardedArray(toks.shape, toks.dtype, toks.sharding, tl).to_torch().long()
            ch = ShardedArray(cnt.shape, cnt.dtype, cnt.sharding, cl).to_torch()
            for b in range(B):
                n = int(ch[b])
                rows[b].append(th[b, :n])
                emitted += n
                rounds += n > 0
    out = torch.stack([torch.cat(r)[:max_new_tokens] for r in rows])
    if out.shape[1] != max_new_tokens:
        raise RuntimeError(f"generate: {out.shape[1]} of {max_new_tokens} tokens after {len(kept)} rounds")
    return out, emitted / max(rounds, 1)


def _sampling_request(V: int, key, temperature, top_k, top_p, eos_id, pad_id, stop_poll):
    """The checks of ``generate``'s sampling arguments, on the host before any launch: the eos ids as a tuple."""
    eos = () if eos_id is None else ((int(eos_id),) if isinstance(eos_id, (int, np.integer)) else
                                     tuple(int(e) for e in eos_id))
    if eos_id is not None and not eos:
        raise ValueError("generate: eos_id must be an int or 1 to 8 ints, got none")
    if eos and pad_id is None:
        raise ValueError("generate: eos_id needs a pad_id (what a finished sequence writes)")
    if int(stop_poll) < 0:
        raise ValueError(f"generate: stop_poll must be >= 0, got {stop_poll}")
    K.sample_params(V, key, temperature, top_k, top_p, eos, 0 if pad_id is None else pad_id, pad_id is not None,
                    "generate")
    return eos


def _generate_sampled(model, params, ids, max_new_tokens, cache, pl, capture, key, temperature, top_k, top_p, eos,
                      pad_id, stop_poll) -> torch.Tensor:
    """``generate`` with a key and / or stop tokens: the prefill and the step end in ``sample_logits``.  ``done`` (int32
    (batch,), next to ``cache.lens``) is made before the capture and donated with the token."""
    from ..spmd.api import jit
    B = ids.shape[0]
    pad = 0 if pad_id is None else int(pad_id)
    opts = dict(temperature=temperature, top_k=top_k, top_p=top_p, eos=eos, pad=pad)
    lens = cache.lens
    done = ShardedArray(lens.shape, lens.dtype, lens.sharding,
                        {d: torch.zeros_like(t) for d, t in lens.local.items()}) if eos else None

    def prefill(p, x, c, n):
        logits, c = model.apply({"params": p}, x, cache=c, prompt_lens=n)
        last = ShardedArray(n.shape, n.dtype, n.sharding, {d: t - 1 for d, t in n.local.items()})
        # pos = lens after the prefill set it: the position the new token will occupy
        return core.sample_logits(logits, None, key, at=last, pos=c.lens, done=done, dtype=x.dtype, **opts), c

    def step(p, st, c):
        logits, c = model.apply({"params": p}, st[0], cache=c)
        core.sample_logits(logits, st[0], key, pos=c.lens, done=st[1] if eos else None, **opts)   # in place
        return st, c

    step_j = jit(step, donate_argnums=(1, 2), capture=capture)
    with torch.no_grad():
        tok, cache = prefill(params, ids, cache, pl)
        st = (tok, done) if eos else (tok,)
        kept = [{d: t.clone() for d, t in tok.local.items()}]
        for s in range(1, max_new_tokens):
            # outside the graph: one host read of done every stop_poll steps
            if eos and stop_poll and s % int(stop_poll) == 0 and all(bool(t.all()) for t in done.local.values()):
                break
            st, cache = step_j(params, st, cache)
            kept.append({d: t.clone() for d, t in st[0].local.items()})
        out = [ShardedArray(tok.shape, tok.dtype, tok.sharding, loc).to_torch().reshape(B, 1) for loc in kept]
    out = torch.cat(out, dim=1).long()
    if out.shape[1] < max_new_tokens:      # every sequence had stopped
        out = torch.cat([out, torch.full((B, max_new_tokens - out.shape[1]), pad, dtype=torch.long)], dim=1)
    return out


def _stop_lens(out: torch.Tensor, eos) -> torch.Tensor:
    """Per sequence, the count of tokens up to and including its first eos (all of them without one)."""
    hit = torch.zeros_like(out, dtype=torch.bool)
    for e in eos:
        hit |= out == e
    n = out.shape[1]
    first = torch.where(hit, torch.arange(n).expand_as(out), n - 1).amin(-1)
    return first + 1


def generate(model, params, ids: ShardedArray, max_new_tokens: int, prompt_lens=None, capture: Optional[bool] = None,
             max_len: Optional[int] = None, cache_sharding: Optional[Sharding] = None, *, key=None,
             temperature: float = 1.0, top_k: Optional[int] = None, top_p: Optional[float] = None, eos_id=None,
             pad_id: Optional[int] = None, stop_poll: int = 16, return_lens: bool = False,
             cache_quant: Optional[str] = None, draft=None, draft_tokens: int = 4):
    """Decoding: ``max_new_tokens`` tokens after each prompt of ``ids`` (batch, T), as an int64 host tensor
    ``[batch, max_new_tokens]``; greedy without a ``key``.

    ``key`` (a ``random.Key``): every token is drawn from the softmax of ``logits / temperature`` restricted by ``top_k``
    and ``top_p`` (:func:`~..ops.kernels.sample_reference` states the rule), the stream id of a draw being (the
    sequence's global batch index, the position the token will occupy): the tokens do not depend on the mesh, on
    ``capture`` or on the batch a sequence is decoded in.  ``eos_id`` (an int or up to 8): a sequence that has
    produced one writes ``pad_id`` from then on; every ``stop_poll`` steps (0: never) the host reads whether all
    sequences have stopped and, if so, ends early, the remaining columns being ``pad_id``.  ``return_lens=True``
    returns ``(tokens, lens)``, ``lens[b]`` the count of tokens up to and including sequence b's eos.  With a key
    or an ``eos_id`` the prefill and the step end in :func:`~..ops.core.sample_logits` on the devices; with neither, in
    the argmax on the devices, as before.  Bad arguments raise ``ValueError`` before any launch.

    ``prompt_lens`` (``batch`` ints in ``[1, T]``): the real length of each right-padded prompt (default: T).
    One prefill call fills the cache and gives the first token (the ``argmax``, on the device, of the
    logits at each sequence's last real position); ``max_new_tokens - 1`` decode steps follow.  The step
    is ``jit(step, donate_argnums=(token, cache), capture=capture)``: on the GPU with ``capture=True`` it is
    captured once and replayed.  The cache holds ``max_len`` rows (default: the model's ``max_len``, else
    ``max(prompt_lens) + max_new_tokens``) and is laid out by ``cache_sharding`` (default: the batch dim
    sharded the way ``ids``' is); a request that does not fit raises ``ValueError`` before any launch.

    ``cache_quant="mxfp8"``: the cache is MX-fp8 (:class:`KVCache`): about half the bytes per cached row, the launch
    count of a step unchanged.  The prefill attends to the prompt's unquantised K / V, so the first token is the
    unquantised run's; the later ones attend to fp8 keys and values and may differ from it.

    ``draft=(draft_model, draft_params)``: greedy speculative decoding.  Per round the draft (a cheaper model of the same
    vocabulary, with a cache and a prefill of its own) proposes ``draft_tokens`` tokens and the target checks them in ONE
    cached call on ``draft_tokens + 1`` positions (``extend=True``), keeping the longest prefix it would have decoded itself
    plus its own next token: the tokens are plain greedy ``generate``'s (a multi-position step has a single step's bits
    wherever its projections do, ``batch * (draft_tokens + 1) <= 16`` on the GPU), in fewer target calls.  The round is
    captured once; the host reads the per-sequence counts every ``stop_poll`` rounds and stops when every sequence has
    its tokens.  Greedy only: with a ``key`` or an ``eos_id``, a draft of another vocabulary, ``draft_tokens`` outside ``[1,
    63]`` or ``max(prompt_lens) + max_new_tokens + draft_tokens > max_len`` it raises ``ValueError`` before any launch.
    ``return_lens=True`` then returns ``(tokens, lens, mean tokens per round and unfinished sequence)``."""
    from ..spmd.api import jit
    from ..sharding.tile import TileAssignment
    if ids.ndim != 2:
        raise ValueError(f"generate: ids must be (batch, length), got shape {tuple(ids.shape)}")
    if max_new_tokens < 1:
        raise ValueError(f"generate: max_new_tokens must be positive, got {max_new_tokens}")
    if cache_quant not in (None, QUANT_MXFP8):
        raise ValueError(f"generate: cache_quant must be None or {QUANT_MXFP8!r}, got {cache_quant!r}")
    B, T = ids.shape
    plens = _host_lens(prompt_lens, B, T)
    spec = _draft_request(model, draft, draft_tokens, key, eos_id) if draft is not None else None
    ahead = spec[2] if spec else 0       # rows a round writes beyond the tokens it may keep
    need = max(plens) + max_new_tokens + ahead
    cap = max_len if max_len is not None else (model.max_len if model.max_len is not None else need)
    if need > cap or T > cap:
        raise ValueError(f"generate: max(prompt_lens) + max_new_tokens{' + draft_tokens' if spec else ''} = {max(plens)} + "
                         f"{max_new_tokens}{f' + {ahead}' if spec else ''} > max_len {cap} (or the padded prompt length {T} "
                         "is)")
    if cache_sharding is None:
        it = ids.tile
        ct = TileAssignment.from_coords({d: (it.coords[d][0], 0, 0, 0) for d in it.device_ids},
                                        (it.tile_shape[0], 1, 1, 1))
        cache_sharding = sharding_from_tile(ct, like=[ids.sharding])
    eos = _sampling_request(model.vocab_size, key, temperature, top_k, top_p, eos_id, pad_id, stop_poll)
    cache = model.init_cache(B, cap, sharding=cache_sharding, **({"quant": cache_quant} if cache_quant else {}))
    pl = device_put(np.asarray(plens, dtype=np.int32), cache.lens.sharding)
    if spec:
        dcache = spec[0].init_cache(B, cap, sharding=cache_sharding, **({"quant": cache_quant} if cache_quant else {}))
        out, mean = _generate_speculative(model, params, spec[0], spec[1], spec[2], ids, plens, max_new_tokens, cache,
                                          dcache, pl, capture, stop_poll)
        return (out, torch.full((B,), max_new_tokens, dtype=torch.long), mean) if return_lens else out
    if key is not None or eos:
        out = _generate_sampled(model, params, ids, max_new_tokens, cache, pl, capture, key, temperature, top_k, top_p,
                                eos, pad_id, stop_poll)
        return (out, _stop_lens(out, eos)) if return_lens else out

    def prefill(p, x, c, n):
        logits, c = model.apply({"params": p}, x, cache=c, prompt_lens=n)
        last = ShardedArray(n.shape, n.dtype, n.sharding, {d: t - 1 for d, t in n.local.items()})
        return _greedy(logits, x, last), c

    def step(p, tok, c):
        logits, c = model.apply({"params": p}, tok, cache=c)
        new = _greedy(logits, tok)
        for d, t in tok.local.items():     # in place: the next call passes the very same buffers
            t.copy_(new.local[d])
        return tok, c

    step_j = jit(step, donate_argnums=(1, 2), capture=capture)
    with torch.no_grad():
        tok, cache = prefill(params, ids, cache, pl)
        out = [tok.to_torch().clone()] if max_new_tokens == 1 else []
        if max_new_tokens > 1:
            # the step's token buffers are rewritten at every step: keep a copy of each, on the devices
            kept = [{d: t.clone() for d, t in tok.local.items()}]
            for _ in range(max_new_tokens - 1):
                tok, cache = step_j(params, tok, cache)
                kept.append({d: t.clone() for d, t in tok.local.items()})
            out = [ShardedArray(tok.shape, tok.dtype, tok.sharding, loc).to_torch() for loc in kept]
    out = torch.cat([t.reshape(B, 1) for t in out], dim=1).long()
    return (out, torch.full((B,), max_new_tokens, dtype=torch.long)) if return_lens else out
