"""CLI generation drivers for the transformer families (GPT-2 / Llama-3).

The reference's GPT stages exist only as modules (``partitions/
gpt_model_parts.py:6-50``) that recompute the whole prefix per call; nothing
drives them (``node.py`` registers CIFAR parts only, ``node.py:29-32``).  Here
the config's ``micro_batch_size`` x ``num_microbatches`` sequences are decoded
greedily (or sampled) through the pipeline with the ``DecodeRing`` schedule
(``runtime/scheduler.py``):

* ``run_generate_colocated`` — every stage on one GPU (one ring group, each
  microbatch's decode step one HIP graph);
* ``run_generate_dist`` — one rank per stage over RCCL / gloo, tokens return to
  stage 0 over the back-edge.

Stage 0 prints the reference's ``***** FINAL PREDICTION (Index): k *****`` line
(first generated token of the first sequence), the generated tokens, and one
``METRICS`` JSON line with prefill / decode token rates.
"""
from __future__ import annotations

import json
import math
import time
from typing import List, Optional

import torch

from ..models import model_info
from ..utils.log import log
from .scheduler import DecodeRing, RingLinks


def prompt_lists(pipe, prompt: Optional[str]):
    """The prompts the run was given, validated (``config.make_prompt_lists``):
    ``--prompt`` (comma-separated ids, ``;`` between prompts:
    ``"464,2068,7586;40;11,12"``), else the config's ``prompts``, else None
    (random ids).  ``--prompt`` overrides the config key."""
    from ..config import ConfigError, make_prompt_lists
    if not prompt:
        return pipe.prompts
    try:
        given = [[int(v) for v in q.split(",") if v.strip()] for q in prompt.split(";")]
    except ValueError:
        raise ConfigError(f"ERROR: '--prompt' must hold comma-separated integers, ';' between prompts, got {prompt!r}")
    return make_prompt_lists(model_info(pipe.model).cfg.vocab_size, given,
                             pipe.micro_batch_size * pipe.num_microbatches, key="--prompt")


def pad_id(pipe) -> int:
    """What fills a shorter prompt up to the longest: the config's
    ``pad_token_id`` when it has one, else 0."""
    v = (pipe.raw or {}).get("pad_token_id")
    return int(v) if v is not None else 0


def make_prompt_batch(pipe, prompt: Optional[str], replica: int = 0):
    """``(ids, lens)``: (micro_batch_size * num_microbatches, T) int64 prompt
    ids and the (n,) int32 prompt lengths, or None when all are equal (the
    ring then runs its equal-length path).  Sequence i takes prompt
    ``i % n_prompts`` of ``prompt_lists``, right-padded to the longest with
    ``pad_id``; without prompts, seeded random ids (each data-parallel replica
    draws its own batch)."""
    info = model_info(pipe.model)
    n = pipe.micro_batch_size * pipe.num_microbatches
    given = prompt_lists(pipe, prompt)
    if given is None:
        g = torch.Generator().manual_seed(1234 + 7919 * replica)
        T = pipe.prompt_len or pipe.seq_len
        return torch.randint(0, info.cfg.vocab_size, (n, T), generator=g), None
    T = max(len(q) for q in given)
    ids = torch.full((n, T), pad_id(pipe), dtype=torch.int64)
    lens = torch.empty((n,), dtype=torch.int32)
    for i in range(n):
        q = given[i % len(given)]
        ids[i, :len(q)] = torch.tensor(q, dtype=torch.int64)
        lens[i] = len(q)
    return ids, (lens if int(lens.min()) != T else None)


def make_prompts(pipe, prompt: Optional[str], replica: int = 0) -> torch.Tensor:
    """The ids of ``make_prompt_batch`` alone."""
    return make_prompt_batch(pipe, prompt, replica)[0]


def kv_capacity(pipe, T: int) -> tuple:
    """(sequences, positions) every stage's KV cache must hold."""
    return pipe.micro_batch_size * pipe.num_microbatches, T + max(1, pipe.decode_steps or 1)


def check_capacity(stages, n_seq: int, n_pos: int) -> None:
    for s in stages:
        mb, ms = getattr(s, "max_batch", None), getattr(s, "max_seq", None)
        if mb is not None and mb < n_seq:
            raise ValueError(f"stage KV cache holds {mb} sequences, the run needs {n_seq}")
        if ms is not None and ms < n_pos:
            raise ValueError(f"stage KV cache holds {ms} positions, the run needs {n_pos} (prompt + decode steps)")
        bs = getattr(getattr(s, "cfg", None), "block_size", None)
        if bs is not None and n_pos > bs:
            raise ValueError(f"prompt + decode steps = {n_pos} exceeds the model's block_size {bs}")


def penalties_on(pipe) -> bool:
    """The config asks for a repetition / presence / frequency penalty: the last
    stage then needs every prompt's token ids (``DecodeRing(forward_prompt_ids=)``)."""
    return pipe.repetition_penalty != 1.0 or pipe.presence_penalty != 0.0 or pipe.frequency_penalty != 0.0


def needs_prompt_ids(pipe) -> bool:
    """The last stage needs every prompt's token ids: for the penalties, or for
    logit constraints that read the rows' context (``no_repeat_ngram_size``, a
    bad word longer than one token)."""
    cons = getattr(pipe, "constraints", None)
    return penalties_on(pipe) or (cons is not None and cons.needs_context)


def _sync(dev):
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)


def _report(nid: str, toks: torch.Tensor, prefill_s: float, decode_s: float, n_seq: int, T: int, steps: int,
            M: int, groups: int, lens: Optional[torch.Tensor] = None) -> None:
    first = toks[:, 0].tolist()
    log(f"[{nid}] ***** FINAL PREDICTION (Index): {first[0] if len(first) == 1 else first} *****")
    log(f"[{nid}] generated tokens: {json.dumps(toks.tolist())}")
    log("METRICS " + json.dumps(metrics(nid, prefill_s, decode_s, n_seq, T, steps, M, groups, lens)))


def metrics(nid: str, prefill_s: float, decode_s: float, n_seq: int, T: int, steps: int, M: int, groups: int,
            lens: Optional[torch.Tensor] = None) -> dict:
    """The ``METRICS`` record of one generation: ``prompt_len`` is the longest
    prompt, ``prompt_tokens`` the sum of all lengths (what
    ``prefill_tokens_per_s`` counts: pads are no tokens) and, when the lengths
    differ, ``prompt_lens`` the lengths themselves."""
    n_prompt = int(lens.sum()) if lens is not None else n_seq * T
    m = {"node": nid, "sequences": n_seq, "microbatches": M, "ring_groups": groups, "prompt_len": T,
         "prompt_tokens": n_prompt, "decode_steps": steps - 1,
         "prefill_tokens_per_s": round(n_prompt / prefill_s, 1) if prefill_s > 0 else None,
         "decode_tokens_per_s": round(n_seq * (steps - 1) / decode_s, 1) if steps > 1 and decode_s > 0 else None,
         "decode_ms_per_step": round(decode_s / (steps - 1) * 1e3, 4) if steps > 1 else None}
    if lens is not None:
        m["prompt_lens"] = lens.tolist()
    return m


def _report_logprobs(nid: str, ring: DecodeRing) -> None:
    """One ``LOGPROBS {...}`` JSON line from the rank that holds them (the last
    stage's; config key ``logprobs``): every sequence's chosen log-probabilities,
    aligned with the ``generated tokens`` line, and the first sequence's top-n
    (``DNN_LOGPROBS_ALL=1``: also every sequence's, as ``top_ids`` /
    ``top_logprobs``).  The numbers are the fp32 values, written so that they
    read back exactly; -inf and NaN, which JSON lacks, are null."""
    if ring.lp_chosen is None:
        return
    import os

    def fin(t):
        if isinstance(t, list):
            return [fin(v) for v in t]
        return t if math.isfinite(t) else None
    lp = ring.logprobs()
    rec = {"node": nid, "n": int(lp["top_ids"].shape[2]), "chosen": fin(lp["chosen"].tolist()),
           "top_ids_seq0": lp["top_ids"][0].tolist(), "top_logprobs_seq0": fin(lp["top_lps"][0].tolist())}
    if os.environ.get("DNN_LOGPROBS_ALL") == "1":
        rec["top_ids"] = lp["top_ids"].tolist()
        rec["top_logprobs"] = fin(lp["top_lps"].tolist())
    log("LOGPROBS " + json.dumps(rec))


def _report_finish(nid: str, ring: DecodeRing) -> None:
    """One ``FINISH {...}`` JSON line from the rank that holds the last stage
    (config keys ``eos_token_id`` / ``stop_token_ids`` / ``stop_sequences``):
    every sequence's number of valid tokens in the ``generated tokens`` line
    (the rest of its row is ``pad_token_id``) and why it ended: null (it never
    stopped), ``["token", index]`` or ``["sequence", index]``."""
    if ring.stp is None:
        return
    fin = ring.finished()
    log("FINISH " + json.dumps({"node": nid, "pad_token_id": ring.stp.stop.pad_token_id,
                                "length": fin["length"].tolist(),
                                "reason": [None if r is None else list(r) for r in fin["reason"]]}))


def _timed_generate(ring: DecodeRing, prompts, T: int, steps: int, dev, chunk: int = 0, lens=None):
    """(prefill seconds, decode seconds, tokens per sequence): the last is
    ``steps`` unless the ring left early because every sequence had stopped."""
    t0 = time.perf_counter()
    ring.prefill(prompts, T, chunk, lens)
    if steps > 1:
        ring.capture()
    _sync(dev)
    t1 = time.perf_counter()
    ran = ring.decode_rounds(steps - 1) if steps > 1 else 0
    ring.drain()
    _sync(dev)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, 1 + ran


def run_generate_colocated(ctx, args, stages: List, device) -> int:
    pipe = ctx.pipeline
    prompt, lens = make_prompt_batch(pipe, args.prompt)
    n_seq, T = prompt.shape
    steps = max(1, pipe.decode_steps or 1)
    check_capacity(stages, *kv_capacity(pipe, T))
    M, B = pipe.num_microbatches, pipe.micro_batch_size
    ring = DecodeRing(stages, RingLinks(), 1, M, B)
    prompts = [prompt[m * B:(m + 1) * B] for m in range(M)]
    mlens = [lens[m * B:(m + 1) * B] for m in range(M)] if lens is not None else None
    pf, dec, steps = _timed_generate(ring, prompts, T, steps, device, pipe.prefill_chunk, mlens)
    _report(ctx.node_id, ring.tokens(), pf, dec, n_seq, T, steps, M, 1, lens)
    _report_logprobs(ctx.node_id, ring)
    _report_finish(ctx.node_id, ring)
    return 0


def run_generate_dist(ctx, args, stage, info, progress=None) -> int:
    """One rank per stage; tokens return to stage 0 over the back-edge.  The
    prompt shape travels down the chain in a header from stage 0; its kind
    says whether per-sequence prompt lengths follow (``KIND_RAGGED``: only
    stage 0 sees ``--prompt``, so no other rank may rely on its own command
    line)."""
    from ..parallel import comm
    from ..parallel.links import KIND_DATA, KIND_RAGGED, make_link
    pipe = ctx.pipeline
    S, r, dev = pipe.num_parts, ctx.part_index, info.device
    peer = getattr(ctx, "peer", lambda p: p)  # ranks of this replica's stages
    if pipe.return_to_node_id and pipe.by_id(pipe.return_to_node_id) and \
            pipe.by_id(pipe.return_to_node_id).part_index != 0 and r == S - 1:
        log(f"[{ctx.node_id}] note: generated tokens feed the embedding, so they return to stage 0 "
            f"(return_to_node_id '{pipe.return_to_node_id}' is not stage 0)")
    bg = comm.back_group()  # the token back-edge on its own communicator / stream
    links = RingLinks(prev=make_link(peer(r - 1), dev) if r > 0 else None,
                      nxt=make_link(peer(r + 1), dev) if r < S - 1 else None,
                      back_out=make_link(peer(0), dev, bg) if (r == S - 1 and S > 1) else None,
                      back_in=make_link(peer(S - 1), dev, bg) if (r == 0 and S > 1) else None)
    M, B = pipe.num_microbatches, pipe.micro_batch_size
    steps = max(1, pipe.decode_steps or 1)
    prompts = lens = mlens = None
    if r == 0:
        prompt, lens = make_prompt_batch(pipe, args.prompt, getattr(ctx, "replica", 0))
        T = prompt.shape[1]
        prompts = [prompt[m * B:(m + 1) * B] for m in range(M)]
        mlens = [lens[m * B:(m + 1) * B] for m in range(M)] if lens is not None else None
        kind = KIND_RAGGED if lens is not None else KIND_DATA
    else:
        kind, _, T, steps = links.prev.recv_header()
    if links.nxt is not None:
        links.nxt.send_header(kind, B, T, steps)
    check_capacity([stage], *kv_capacity(pipe, T))
    ring = DecodeRing([stage], links, S, M, B, progress=progress, forward_prompt_ids=needs_prompt_ids(pipe),
                      ragged=kind == KIND_RAGGED)
    pf, dec, steps = _timed_generate(ring, prompts, T, steps, dev, pipe.prefill_chunk, mlens)
    if r == 0:
        nid = ctx.node_id + (f" replica {ctx.replica}" if getattr(pipe, "replicas", 1) > 1 else "")
        _report(nid, ring.tokens(), pf, dec, B * M, T, steps, M, S, lens)
    _report_logprobs(ctx.node_id, ring)  # the last rank's: nothing new travels over the back-edge
    _report_finish(ctx.node_id, ring)  # likewise: the padded tokens are all that travels
    return 0
