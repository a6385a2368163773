"""Logit constraints on the CPU: the config keys, the torch mirror
(runtime/sampling.py constraints_ref) against a plain Python loop written from
the rules, the named edge cases, TorchStage rings against a full-prefix host
loop that applies the plain-loop rules, and two gloo ranks against one process."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

from distributed_neural_networks_amd.config import (CON_MAX_BAD_LEN, CON_MAX_BAD_WORDS, CON_MAX_BIAS, CON_MAX_NGRAM,
                                                    ConfigError, ConstraintConfig, StopConfig, make_constraints,
                                                    parse_pipeline)
from distributed_neural_networks_amd.runtime.sampling import (apply_penalties_ref, constraints_ref,
                                                              constraints_store_prev, logprobs_ref, penalty_count,
                                                              penalty_state, pick, stop_ref, stop_state)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
NEG = 0xFF80  # bf16 -inf


# ---------------------------------------------------------------------- the third implementation: a plain loop
def _bf2f(bits):
    return np.float32(struct.unpack("<f", struct.pack("<I", (bits & 0xFFFF) << 16))[0])


def _f2bf(f):
    """fp32 -> bf16 bits, round to nearest even; NaN stays NaN."""
    u = struct.unpack("<I", struct.pack("<f", float(f)))[0]
    if (u & 0x7FFFFFFF) > 0x7F800000:
        return (u >> 16) | 0x40
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF


def loop_rules(bits, c, bias=(), allowed=None, bad=(), n=0):
    """One row.  ``bits``: the bf16 logits as 16-bit integers; ``c``: the row's
    context (prompt, then generated tokens).  Returns the new bits."""
    V, L = len(bits), len(c)
    out = list(bits)
    with np.errstate(all="ignore"):
        for i, b in bias:
            out[i] = _f2bf(np.float32(_bf2f(out[i]) + np.float32(b)))
    if allowed is not None:
        for i in range(V):
            if i not in allowed:
                out[i] = NEG
    for s in bad:
        k = len(s)
        if L >= k - 1 and list(c[L - (k - 1):L]) == list(s[:k - 1]):
            out[s[k - 1]] = NEG
    if n > 0:
        for j in range(L):
            if j + n - 1 <= L - 1 and list(c[j:j + n - 1]) == list(c[L - n + 1:L]):
                t = c[j + n - 1]
                if 0 <= t < V:
                    out[t] = NEG
    return out


def _bits(x):
    return (x.to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF)


def _from_bits(rows):
    t = torch.tensor(rows, dtype=torch.int32)
    return torch.where(t >= 0x8000, t - 0x10000, t).to(torch.int16).view(torch.bfloat16)


def loop_apply(logits, cons, contexts):
    """``loop_rules`` on every row of ``logits`` (rounded to bf16): bf16 (M, V)."""
    b = _bits(logits).tolist()
    allowed = None if cons.allowed_token_ids is None else set(cons.allowed_token_ids)
    return _from_bits([loop_rules(b[r], contexts[r], cons.logit_bias, allowed, cons.bad_words_ids,
                                  cons.no_repeat_ngram_size) for r in range(len(b))])


def mirror_apply(logits, cons, contexts, width=None, poison=None, prev=False):
    """``constraints_ref`` on the same rows, the contexts as a padded table;
    ``prev``: the newest token is left out of the table and passed as ``prev``."""
    lens = [len(c) for c in contexts]
    width = width or max(lens + [1])
    fill = -1 if poison is None else poison
    tab = torch.full((len(contexts), width), fill, dtype=torch.int32)
    pv = torch.full((len(contexts),), -1, dtype=torch.int32)
    for r, c in enumerate(contexts):
        keep = c[:-1] if (prev and c) else c
        tab[r, :len(keep)] = torch.tensor(keep, dtype=torch.int32)
        if prev and c:
            pv[r] = c[-1]
    return constraints_ref(logits, cons, tab, lens, pv if prev else None)


def same(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------- config keys
V0 = 512


def test_config_normal_forms():
    c = make_constraints(V0, logit_bias={"7": -1.5, 9: 2, " 11 ": 0.25}, allowed_token_ids=[1, 2, 7],
                         bad_words_ids=[[3], [4, 5, 6]], no_repeat_ngram_size=3)
    assert c == ConstraintConfig(((7, -1.5), (9, 2.0), (11, 0.25)), (1, 2, 7), ((3,), (4, 5, 6)), 3)
    assert c.needs_context
    c = make_constraints(V0, logit_bias=[[7, -1.5], (9, 2)])
    assert c.logit_bias == ((7, -1.5), (9, 2.0)) and not c.needs_context and c.allowed_token_ids is None
    assert not make_constraints(V0, bad_words_ids=[[3], [5]]).needs_context
    assert make_constraints(V0, bad_words_ids=[[3, 4]]).needs_context
    assert make_constraints(V0, no_repeat_ngram_size=1).needs_context
    assert make_constraints(V0, logit_bias={str(i): 100.0 for i in range(CON_MAX_BIAS)}) is not None
    assert make_constraints(V0, bad_words_ids=[[1] * CON_MAX_BAD_LEN] * CON_MAX_BAD_WORDS) is not None
    assert make_constraints(V0, no_repeat_ngram_size=CON_MAX_NGRAM).no_repeat_ngram_size == 16
    assert (CON_MAX_BIAS, CON_MAX_BAD_WORDS, CON_MAX_BAD_LEN, CON_MAX_NGRAM) == (256, 64, 16, 16)


def test_neutral_config_yields_none():
    assert make_constraints(V0) is None
    assert make_constraints(V0, logit_bias={}, bad_words_ids=[], no_repeat_ngram_size=0) is None
    assert make_constraints(V0, logit_bias=[]) is None
    base = _cfg()
    assert parse_pipeline(base).constraints is None
    base.update({"logit_bias": None, "allowed_token_ids": None, "bad_words_ids": None, "no_repeat_ngram_size": 0})
    assert parse_pipeline(base).constraints is None


@pytest.mark.parametrize("kw,msg", [
    (dict(logit_bias=3), "logit_bias"),
    (dict(logit_bias=[[1, 2, 3]]), "logit_bias"),
    (dict(logit_bias={"x": 1.0}), "no token id"),
    (dict(logit_bias={"-1": 1.0}), "outside"),
    (dict(logit_bias={str(V0): 1.0}), "outside"),
    (dict(logit_bias={"1": float("inf")}), "finite"),
    (dict(logit_bias={"1": float("nan")}), "finite"),
    (dict(logit_bias={"1": 100.5}), "finite"),
    (dict(logit_bias={"1": -101}), "finite"),
    (dict(logit_bias={"1": "2"}), "finite"),
    (dict(logit_bias={"1": True}), "finite"),
    (dict(logit_bias=[[1, 1.0], [1, 2.0]]), "distinct"),
    (dict(logit_bias={"1": 1.0, 1: 2.0}), "distinct"),
    (dict(logit_bias={str(i): 1.0 for i in range(CON_MAX_BIAS + 1)}), "at most 256"),
    (dict(allowed_token_ids=[]), "must not be empty"),
    (dict(allowed_token_ids=[1, 1]), "distinct"),
    (dict(allowed_token_ids=[V0]), "outside"),
    (dict(allowed_token_ids=[-1]), "outside"),
    (dict(allowed_token_ids=5), "list of integers"),
    (dict(allowed_token_ids=[1.5]), "list of integers"),
    (dict(bad_words_ids=[1, 2]), "list of lists"),
    (dict(bad_words_ids=[[]]), "1..16"),
    (dict(bad_words_ids=[[1] * 17]), "1..16"),
    (dict(bad_words_ids=[[1]] * 65), "at most 64"),
    (dict(bad_words_ids=[[V0]]), "outside"),
    (dict(bad_words_ids=[[True]]), "list of integers"),
    (dict(no_repeat_ngram_size=-1), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=17), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=2.0), "no_repeat_ngram_size"),
    (dict(no_repeat_ngram_size=True), "no_repeat_ngram_size"),
    (dict(allowed_token_ids=[1, 2], bad_words_ids=[[2], [1], [3, 4]]), "nothing could be generated"),
])
def test_config_rejections(kw, msg):
    with pytest.raises(ConfigError, match=msg):
        make_constraints(V0, **kw)
    c = _cfg()
    c.update(kw)
    with pytest.raises(ConfigError, match=msg):  # ... through the config file's path too, before any weight loads
        parse_pipeline(c)


def _cfg(model="gpt2-tiny", **kw):
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{50300 + i}", "part_index": i} for i in range(2)],
         "model_weights": "synthetic:1", "num_parts": 2, "return_to_node_id": "node1", "transport": "gloo",
         "model": model, "seq_len": 12, "decode_steps": 8, "micro_batch_size": 2, "num_microbatches": 2}
    c.update(kw)
    return c


def test_config_file_keys_and_legal_combinations():
    p = parse_pipeline(_cfg(logit_bias={"7": -1.5}, allowed_token_ids=[1, 2, 7], bad_words_ids=[[2], [4, 5]],
                            no_repeat_ngram_size=2))
    assert p.constraints == ConstraintConfig(((7, -1.5),), (1, 2, 7), ((2,), (4, 5)), 2)
    # allowed ids that exclude every stop id, with min_new_tokens: legal
    p = parse_pipeline(_cfg(allowed_token_ids=[1, 2], eos_token_id=9, min_new_tokens=3))
    assert p.constraints.allowed_token_ids == (1, 2) and p.stop.stop_token_ids == (9,)
    # an allowed id left over next to one-token bad words: legal
    assert make_constraints(V0, allowed_token_ids=[1, 2], bad_words_ids=[[1]]) is not None
    # generating models only
    c = _cfg(model="cifar10")
    for k, v in (("logit_bias", {"1": 1.0}), ("allowed_token_ids", [1]), ("bad_words_ids", [[1]]),
                 ("no_repeat_ngram_size", 2)):
        with pytest.raises(ConfigError, match="generating models only"):
            parse_pipeline(dict(c, **{k: v}))


def test_shipped_config_parses():
    from distributed_neural_networks_amd.config import load_json
    p = parse_pipeline(load_json(os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_constrained.json")))
    c = p.constraints
    assert c.logit_bias and c.allowed_token_ids and c.bad_words_ids and c.no_repeat_ngram_size > 0
    assert any(len(s) == 1 for s in c.bad_words_ids) and any(len(s) > 1 for s in c.bad_words_ids)
    assert p.temperature > 0


# ---------------------------------------------------------------------- the mirror against the plain loop
VS, ALPHA, WIDTH = 12, 5, 40


def _logits(M, V, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((M, V), generator=g) * 3).to(torch.bfloat16)


@pytest.mark.parametrize("n", [1, 2, 3, 16])
def test_mirror_equals_loop_on_random_contexts(n):
    g = torch.Generator().manual_seed(100 + n)
    lens = sorted({0, n - 1, n, n + 1, WIDTH})
    fired = 0
    for trial in range(6):
        contexts = [torch.randint(0, ALPHA, (L,), generator=g).tolist() for L in lens]
        if n == 16:  # a 15-token repeat does not happen by chance: plant one in the full row
            contexts[-1][WIDTH - 15:] = contexts[-1][3:18]
        x = _logits(len(lens), VS, trial)
        bad = tuple(tuple(torch.randint(0, ALPHA, (k,), generator=g).tolist()) for k in (1, 2, 3, 2))
        for cons in (ConstraintConfig((), None, (), n),
                     ConstraintConfig((), None, bad, 0),
                     ConstraintConfig(((1, 2.5), (7, -3.0)), (0, 1, 2, 3, 7, 9), bad, n)):
            want = loop_apply(x, cons, contexts)
            for kw in (dict(), dict(width=WIDTH, poison=11), dict(prev=True, width=WIDTH)):
                got = mirror_apply(x, cons, contexts, **kw)
                assert got.dtype == torch.bfloat16 and same(got, want), (n, trial, cons, kw)
            if cons.bad_words_ids == () and cons.allowed_token_ids is None:
                fired += int((_bits(want) != _bits(x)).any())
                assert same(want[0], x[0]) or lens[0] >= n  # len < n bans nothing
                for r, L in enumerate(lens):
                    if L < n:
                        assert same(want[r], x[r])
    assert fired >= 1  # never vacuous: the n-gram rule banned something


def test_named_edge_cases():
    x = _logits(1, VS, 3)
    xb = _bits(x)[0].tolist()

    def run(c, **kw):
        cons = ConstraintConfig(kw.get("bias", ()), kw.get("allowed"), kw.get("bad", ()), kw.get("n", 0))
        want = loop_apply(x, cons, [c])
        assert same(mirror_apply(x, cons, [c]), want)
        if c and 0 <= c[-1] < VS:  # the newest token through `prev` (one outside [0, V) is never stored)
            assert same(mirror_apply(x, cons, [c], prev=True, width=30), want)
        return _bits(want)[0].tolist()

    def banned(out):
        return {i for i in range(VS) if out[i] == NEG and xb[i] != NEG}

    # a match at j = 0: c = [1 2 5 ... 1 2] bans 5
    assert banned(run([1, 2, 5, 9, 9, 1, 2], n=3)) == {5}
    # a match at the last legal j (j + n - 1 = len - 1): the banned token is the newest one
    assert banned(run([4, 7, 7], n=2)) == {7}
    assert banned(run([3, 4, 6, 4], n=2)) == {6}
    # the suffix does not match itself: [1 2 3] has no earlier "2 3" window, nothing is banned
    assert banned(run([1, 2, 3], n=3)) == set()
    assert banned(run([1, 2], n=3)) == set() and banned(run([], n=1)) == set()
    # n = 1 bans every token of the context
    assert banned(run([3, 3, 8, 0], n=1)) == {0, 3, 8}
    # a one-token bad word: at every step, whatever the context
    assert banned(run([], bad=((6,),))) == {6} and banned(run([1, 2, 3], bad=((6,),))) == {6}
    # a bad word whose prefix spans the prompt / generation boundary: context = prompt [.. 4] + generated [5]
    assert banned(run([9, 4, 5], bad=((4, 5, 6),))) == {6}
    assert banned(run([9, 4], bad=((4, 5, 6),))) == set() and banned(run([5], bad=((4, 5, 6),))) == set()
    # bias on a banned entry: the ban wins
    out = run([3], bias=((3, 50.0),), n=1)
    assert out[3] == NEG
    out = run([], bias=((3, 50.0),), allowed=(1, 2))
    assert out[3] == NEG and out[1] == xb[1]
    # ids outside [0, V) in the context are compared, never indexed
    assert banned(run([100, -7, 2, 100, -7], n=3)) == {2}
    assert banned(run([1, 100, 1], n=2)) == set()  # the banned token would be 100: nothing to write
    assert banned(run([-1, -1], n=1)) == set()
    # bias on +-inf and +-0
    special = _from_bits([[0x7F80, 0xFF80, 0x0000, 0x8000, 0x3F80, 0x7F7F] + [0] * (VS - 6)])
    cons = ConstraintConfig(tuple((i, b) for i, b in enumerate((5.0, 5.0, 0.0, 0.0, -1.0, 100.0))), None, (), 0)
    want = loop_apply(special, cons, [[]])
    assert same(constraints_ref(special, cons), want)
    assert _bits(want)[0, :6].tolist() == [0x7F80, 0xFF80, 0x0000, 0x0000, 0x0000, 0x7F7F]
    cons = ConstraintConfig(((2, -0.0), (3, -0.0)), None, (), 0)
    assert _bits(constraints_ref(special, cons))[0, 2:4].tolist() == [0x0000, 0x8000]


def test_bias_rounds_once_to_nearest_even():
    # 1.0 + 2^-8 lies halfway between two bf16 values: ties go to the even mantissa
    x = _from_bits([[0x3F80, 0x3F81] + [0] * 6])
    cons = ConstraintConfig(((0, 2.0 ** -8), (1, 2.0 ** -8)), None, (), 0)
    got = _bits(constraints_ref(x, cons))[0, :2].tolist()
    assert got == [0x3F80, 0x3F82] and same(constraints_ref(x, cons), loop_apply(x, cons, [[]]))


def test_store_prev_and_argument_checks():
    tab = torch.full((3, 4), -1, dtype=torch.int32)
    out = constraints_store_prev(tab, [1, 4, 5], [7, VS, 3], VS)
    assert out.tolist() == [[7, -1, -1, -1], [-1] * 4, [-1] * 4] and tab.eq(-1).all()
    with pytest.raises(ValueError, match="need ctx"):
        constraints_ref(_logits(1, VS, 0), ConstraintConfig((), None, (), 2))
    x = _logits(2, VS, 0)
    assert same(constraints_ref(x, ConstraintConfig((), None, ((1,),), 0)), loop_apply(
        x, ConstraintConfig((), None, ((1,),), 0), [[], []]))


# ---------------------------------------------------------------------- TorchStage rings against a host loop
PAD = 3


def _model(model, seed=5):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import build_golden_stage, default_ranges, model_info
    ranges = default_ranges(model, 2)
    sds = [ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, seed) for i, (a, b) in enumerate(ranges)]
    golden = []
    for i, (a, b) in enumerate(ranges):
        gm = build_golden_stage(model, a, b, i == 0, i == 1)
        gm.load_state_dict(sds[i])
        golden.append(gm.eval())
    return ranges, sds, golden, model_info(model).cfg.vocab_size


def _batch(V, lens, seed=11):
    g = torch.Generator().manual_seed(seed)
    T = max(lens)
    ids = torch.randint(0, V - 1, (len(lens), T), generator=g)
    ids = torch.where(ids >= PAD, ids + 1, ids)
    for b, L in enumerate(lens):
        ids[b, L:] = PAD
    return ids


def _ring(model, ranges, sds, samp, M, B):
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    stages = [TorchStage(model, sds[i], a, b, i == 0, i == 1, sampling=samp) for i, (a, b) in enumerate(ranges)]
    return DecodeRing(stages, RingLinks(), 1, M, B, use_graphs=False, early_exit=False)


def host_loop(golden, V, ids, lens, B, steps, samp, first_step=0):
    """Each row on its own unpadded prompt: a full-prefix forward of the golden
    modules per token; the logits rounded to bf16 take the penalties (mirror),
    the constraints (the plain loop, on the row's prompt + output so far), the
    suppression, the pick, the log-probabilities and the stop conditions."""
    temp, top_k, seed, top_p, min_p, rep, pres, freq, nlp, stop, cons = samp
    pen = rep != 1.0 or pres != 0.0 or freq != 0.0
    toks, chosen, top_ids, fin = [], [], [], []
    for m0 in range(0, len(lens), B):
        seqs = [ids[b, :lens[b]].tolist() for b in range(m0, m0 + B)]
        state = torch.cat([penalty_state(torch.tensor([q]), V) for q in seqs], 0) if pen else None
        st = stop_state(B) if stop is not None else None
        prev, out, lp_c, lp_i = None, [], [], []
        for k in range(steps):
            rows = []
            with torch.no_grad():
                for q in seqs:
                    h = torch.tensor([q], dtype=torch.int64)
                    for gm in golden:
                        h = gm(h)
                    rows.append(h[0, -1])
            logits = torch.stack(rows, 0)
            if pen:
                if k > 0:
                    state = penalty_count(state, prev)
                logits = apply_penalties_ref(logits, state, rep, freq, pres)
            if cons is not None:
                logits = loop_apply(logits, cons, seqs)
            if stop is not None and stop.min_new_tokens > 0 and stop.stop_token_ids:
                from distributed_neural_networks_amd.runtime.sampling import stop_suppress_ref
                logits = stop_suppress_ref(logits, st, stop.stop_token_ids, stop.min_new_tokens)
            step = (torch.full((B,), first_step, dtype=torch.int32) if k == 0
                    else torch.tensor([len(q) - 1 for q in seqs], dtype=torch.int32))
            pred = pick(logits, temp, top_k, seed, step, top_p=top_p, min_p=min_p).to(torch.int32)
            prev = pred.clone()
            if nlp:
                c, ti, _ = logprobs_ref(logits, pred, nlp)
                lp_c.append(c)
                lp_i.append(ti)
            if stop is not None:
                st, pred = stop_ref(st, pred, stop.stop_token_ids, stop.stop_sequences, stop.min_new_tokens,
                                    stop.pad_token_id)
            out.append(pred)
            for q, t in zip(seqs, pred.tolist()):
                q.append(t)
        toks.append(torch.stack(out, 1))
        if nlp:
            chosen.append(torch.stack(lp_c, 1))
            top_ids.append(torch.stack(lp_i, 1))
        if stop is not None:
            fin.append(st)
    return (torch.cat(toks, 0), torch.cat(chosen, 0) if chosen else None, torch.cat(top_ids, 0) if top_ids else None,
            torch.cat(fin, 0) if fin else None)


def repeats(seq, n, start):
    """Does an n-gram that ends at index >= start occur earlier in ``seq``?"""
    for e in range(max(start, n - 1), len(seq)):
        g = seq[e - n + 1:e + 1]
        if any(seq[j:j + n] == g for j in range(0, e - n + 1)):
            return True
    return False


def ends_bad(seq, bad, start):
    return any(seq[e - len(s) + 1:e + 1] == list(s) for s in bad for e in range(max(start, len(s) - 1), len(seq)))


def choose_constraints(V, ids, lens, free, n=2):
    """From a free run: no_repeat_ngram_size n, a one-token bad word and a
    bad word that spans row 0's prompt / generation boundary, allowed ids =
    everything but two ids the free run produced, and a bias on two ids."""
    rows = [ids[b, :lens[b]].tolist() + free[b].tolist() for b in range(len(lens))]
    gen = free.flatten().tolist()
    common = max(set(gen), key=gen.count)
    bad = ((int(free[1, 1]),), (rows[0][lens[0] - 1], int(free[0, 0])), (int(free[2, 0]), int(free[2, 1]), int(free[2, 2])))
    out = sorted({common, int(free[3, 2])})
    allowed = tuple(i for i in range(V) if i not in out)
    bias = {}
    for i, v in ((int(free[3, 0]), -6.0), (int(free[1, 0]), 1.5), (PAD, 2.0)):
        bias.setdefault(i, v)  # the ids of logit_bias are distinct
    bias = tuple(bias.items())
    return ConstraintConfig(bias, allowed, bad, n), rows, out


LENS_EQ = [7, 7, 7, 7]
LENS_RAG = [1, 9, 5, 4]
STEPS = 7
SAMPLINGS = [(0.0, 0, 0, 1.0, 0.0), (0.9, 40, 3, 0.95, 0.0)]


def _run_ring(model, ranges, sds, samp, ids, lens, ragged, chunk=0, steps=STEPS, M=2, B=2):
    ring = _ring(model, ranges, sds, samp, M, B)
    prompts = [ids[m * B:(m + 1) * B] for m in range(M)]
    ln = [torch.tensor(lens[m * B:(m + 1) * B]) for m in range(M)] if ragged else None
    return ring, ring.generate(prompts, ids.shape[1], steps, chunk, lens=ln)


@pytest.mark.parametrize("variant", ["alone", "combined", "chunked", "ragged"])
@pytest.mark.parametrize("model", ["gpt2-tiny", "llama3-tiny"])
@pytest.mark.parametrize("sampling", SAMPLINGS, ids=["greedy", "sampled"])
def test_ring_equals_host_loop(model, sampling, variant):
    """Two microbatches of two rows.  The constraints come from the free run of
    the same setting, so each of them fires; the ring's tokens equal the host
    loop's, and the invariants hold on prompt + output by plain loops."""
    ranges, sds, golden, V = _model(model)
    ragged = variant == "ragged"
    lens = LENS_RAG if ragged else LENS_EQ
    ids = _batch(V, lens)
    chunk = 3 if variant == "chunked" else 0  # 7 = 3 + 3 + 1: a one-token final piece
    first = 6 if (chunk and not ragged) else 0  # the sampler's step operand of the last piece
    pen = (1.3, 0.2, 0.1) if variant == "combined" else (1.0, 0.0, 0.0)
    nlp = 3 if variant == "combined" else 0
    base = sampling + pen + (nlp, None)
    free = host_loop(golden, V, ids, lens, 2, STEPS, base + (None,), first)[0]
    _, got_free = _run_ring(model, ranges, sds, base, ids, lens, ragged, chunk)
    assert torch.equal(got_free, free)  # the host loop is a faithful reference without the keys
    cons, rows_free, out = choose_constraints(V, ids, lens, free)
    stop = StopConfig((int(free[2, 3]),), (), 0, PAD) if variant == "combined" else None
    samp = sampling + pen + (nlp, stop, cons)
    want_t, want_c, want_i, want_st = host_loop(golden, V, ids, lens, 2, STEPS, samp, first)
    ring, got = _run_ring(model, ranges, sds, samp, ids, lens, ragged, chunk)
    assert torch.equal(got, want_t), (got.tolist(), want_t.tolist())
    assert not torch.equal(got, free)
    length = [STEPS] * 4
    if stop is not None:
        fin = ring.finished()
        length = torch.where(want_st[:, 1] != 0, want_st[:, 1], torch.tensor(STEPS, dtype=torch.int32))
        assert torch.equal(fin["length"], length)
        length = length.tolist()
    if nlp:
        lp = ring.logprobs()
        for b in range(4):  # columns past a row's length are unspecified; the tolerance of tests/test_ragged.py
            k = length[b]
            assert torch.equal(lp["top_ids"][b, :k], want_i[b, :k])
            assert torch.allclose(lp["chosen"][b, :k], want_c[b, :k], rtol=0, atol=1e-4)
            assert bool(torch.isfinite(lp["chosen"][b, :k]).all())  # taken after the constraints: never a banned token
    # the invariants, on prompt + valid output, by plain loops; the free run violates each
    allowed = set(cons.allowed_token_ids)
    for b in range(4):
        seq = ids[b, :lens[b]].tolist() + got[b, :length[b]].tolist()
        assert not repeats(seq, 2, lens[b]), (b, seq)
        assert not ends_bad(seq, cons.bad_words_ids, lens[b]), (b, seq)
        assert all(t in allowed for t in seq[lens[b]:]), (b, seq)
    if variant != "combined":
        assert any(ends_bad(r, cons.bad_words_ids, lens[b]) for b, r in enumerate(rows_free))
        assert any(t in out for r in free.tolist() for t in r)
    if sampling[0] == 0 and variant == "alone":
        assert any(repeats(r, 2, lens[b]) for b, r in enumerate(rows_free)), rows_free  # greedy tiny models loop


def test_ring_second_generation_and_no_context_rules():
    """A second generation on the same ring starts from its own prompts; rules
    that read no context (bias, allowed ids, one-token bad words) keep none."""
    model = "gpt2-tiny"
    ranges, sds, golden, V = _model(model)
    ids, ids2 = _batch(V, LENS_EQ), _batch(V, LENS_EQ, seed=12)
    base = SAMPLINGS[0] + (1.0, 0.0, 0.0, 0, None)
    free = host_loop(golden, V, ids, LENS_EQ, 2, STEPS, base + (None,))[0]
    cons, _, _ = choose_constraints(V, ids, LENS_EQ, free)
    samp = base + (cons,)
    ring, got = _run_ring(model, ranges, sds, samp, ids, LENS_EQ, False)
    again = ring.generate([ids2[:2], ids2[2:]], 7, STEPS)
    assert torch.equal(again, host_loop(golden, V, ids2, LENS_EQ, 2, STEPS, samp)[0])
    assert torch.equal(ring.generate([ids[:2], ids[2:]], 7, STEPS), got)
    flat = ConstraintConfig(cons.logit_bias, cons.allowed_token_ids, (cons.bad_words_ids[0],), 0)
    ring, got = _run_ring(model, ranges, sds, base + (flat,), ids, LENS_EQ, False)
    last = ring.stages[-1]
    assert not last.constraints_need_context and ring.con is None and last._con_ctx == {}
    assert torch.equal(got, host_loop(golden, V, ids, LENS_EQ, 2, STEPS, base + (flat,))[0])
    with pytest.raises(ValueError, match="keeps no context"):
        last.constraint_begin(0, ids[:2])


def test_stage_and_ring_arguments():
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model = "gpt2-tiny"
    ranges, sds, _, V = _model(model)
    cons = ConstraintConfig((), None, (), 2)
    samp = SAMPLINGS[0] + (1.0, 0.0, 0.0, 0, None, cons)
    (a0, b0), (a1, b1) = ranges
    first = TorchStage(model, sds[0], a0, b0, True, False, sampling=samp)
    assert first.constraints is None and not first.constraints_need_context  # only a last stage acts on the keys
    off = TorchStage(model, sds[1], a1, b1, False, True, sampling=samp[:10])
    assert off.constraints is None and not off.constraints_need_context
    on = TorchStage(model, sds[1], a1, b1, False, True, sampling=samp)
    assert on.constraints is cons and on.constraints_need_context
    with pytest.raises(ValueError, match="no constraint_begin"):
        on.step(torch.zeros((3, 256)), 0, 1, 3)
    # a last stage that needs the context on a ring of several groups, without the prompt ids
    with pytest.raises(ValueError, match="forward_prompt_ids=True"):
        DecodeRing([on], RingLinks(), 2, 1, 2, use_graphs=False)
    from distributed_neural_networks_amd.runtime.generate import needs_prompt_ids
    assert needs_prompt_ids(parse_pipeline(_cfg(no_repeat_ngram_size=2)))
    assert needs_prompt_ids(parse_pipeline(_cfg(bad_words_ids=[[1, 2]])))
    assert not needs_prompt_ids(parse_pipeline(_cfg(bad_words_ids=[[1]], logit_bias={"1": 1.0})))
    assert not needs_prompt_ids(parse_pipeline(_cfg()))


# ---------------------------------------------------------------------- two gloo ranks vs one process
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_nodes(cfg, n, timeout=120, env=ENV):
    procs = []
    for i in range(1, n):
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", f"node{i + 1}",
                                       "--config", str(cfg), "--serve_seconds", "90"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        r0 = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                             "--input_image", "none.png", "--shutdown_pipeline"], env=env,
                            capture_output=True, text=True, timeout=timeout)
        outs = []
        for p in procs:
            try:
                outs.append(p.communicate(timeout=60)[0])
            except subprocess.TimeoutExpired:
                p.kill()
                outs.append(p.communicate()[0])
        return r0, outs
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()


def test_cli_two_gloo_ranks_equal_one_process(tmp_path):
    """The last rank keeps the context: the prompt ids travel down the stage
    links (forward_prompt_ids follows the config), the tokens come back over the
    back-edge, and both equal one process with both stages."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.generate import make_prompts
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, steps = "gpt2-tiny", 10
    ranges = default_ranges(model, 2)
    c = _cfg(seq_len=12, decode_steps=steps, temperature=0.8, top_k=20, top_p=0.9, seed=7)
    for i, nd in enumerate(c["nodes"]):
        nd["address"] = f"127.0.0.1:{_free_port()}"
    prompt = make_prompts(parse_pipeline(c), None)

    def one_process(cons):
        samp = (0.8, 20, 7, 0.9, 0.0, 1.0, 0.0, 0.0, 0, None, cons)
        stages = [TorchStage(model, ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 1), a, b, i == 0,
                             i == 1, sampling=samp) for i, (a, b) in enumerate(ranges)]
        ring = DecodeRing(stages, RingLinks(), 1, 2, 2, use_graphs=False, early_exit=False)
        return ring.generate([prompt[:2], prompt[2:]], prompt.shape[1], steps)

    free = one_process(None)
    T = prompt.shape[1]
    c.update({"logit_bias": {str(int(free[3, 0])): -6.0}, "bad_words_ids": [[int(free[1, 1])],
                                                                            [int(prompt[0, T - 1]), int(free[0, 0])]],
              "allowed_token_ids": [i for i in range(512) if i != int(free[2, 2])], "no_repeat_ngram_size": 2})
    cons = parse_pipeline(c).constraints
    want = one_process(cons)
    assert not torch.equal(want, free)
    for b in range(4):
        seq = prompt[b].tolist() + want[b].tolist()
        assert not repeats(seq, 2, T) and not ends_bad(seq, cons.bad_words_ids, T)
        assert int(free[2, 2]) not in want[b].tolist()
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(c))
    r0, outs = _run_nodes(cfg, 2)
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-2000:] + "".join(o[-2000:] for o in outs)
    toks = torch.tensor(json.loads(r0.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    assert torch.equal(toks, want), (toks.tolist(), want.tolist())
