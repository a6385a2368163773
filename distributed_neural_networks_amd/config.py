"""Config loading and validation for the reference ``config.json`` schema.

Behavioural contract (reference ``node.py:222-290``, ``config.json:1-18``):

* ``nodes[{id, address, part_index}]``, ``model_weights``, ``num_parts`` and the
  optional ``return_to_node_id`` keep their meaning and the reference's error
  strings (``node.py:227,230,236,251,257,266,270``).
* The reference hard-rejects ``num_parts != 2`` (``node.py:246-248``).  Here any
  ``num_parts >= 1`` is accepted as long as the ``part_index`` values are a
  permutation of ``0..num_parts-1`` — the only way a pipeline of more than two
  stages (GPT-2 4-stage, Llama-3 8-stage) can be described with this schema.
* Additive optional fields (absent in the reference file, so it still loads):
  top level ``model``, ``dtype``, ``transport``, ``micro_batch_size``,
  ``num_microbatches``, ``seq_len``, ``decode_steps``, ``prompt_len``, ``prompts``, ``temperature``, ``top_k``,
  ``top_p``, ``min_p``, ``seed``, ``repetition_penalty``, ``presence_penalty``, ``frequency_penalty``,
  ``logprobs``, ``eos_token_id``, ``stop_token_ids``, ``stop_sequences``, ``min_new_tokens``,
  ``pad_token_id``, ``logit_bias``, ``allowed_token_ids``, ``bad_words_ids``, ``no_repeat_ngram_size``,
  ``heartbeat_timeout_s``, ``stall_timeout_s``, ``prefill_chunk``, ``replicas``,
  ``kv_cache_dtype``, ``kv_cache_scale``, ``fp8_prefill``, ``input_dtype``, ``input_mean``,
  ``input_std`` (CIFAR: stage 0 takes uint8 images and normalises them by table); per node
  ``layers: [start, end]`` (inclusive, as in
  ``partitions/gpt_model_parts.py:12``) and ``device``.

Nothing here touches torch, so it is cheap to import from the CLI and tests.
"""
from __future__ import annotations

import json
import math
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Tuple

TRANSPORTS = ("grpc", "colocated", "rccl", "gloo", "gloo_gpu")
DIST_TRANSPORTS = ("rccl", "gloo", "gloo_gpu")  # one rank per stage (and replica)
MODELS = ("cifar10", "gpt2", "gpt2-medium", "gpt2-large", "gpt2-xl", "gpt2-tiny",
          "llama3-8b", "llama3-tiny")


class ConfigError(Exception):
    """A config problem the CLI reports as ``print(msg); exit(1)`` (reference style)."""


@dataclass
class NodeSpec:
    id: str
    address: str
    part_index: int
    layers: Optional[Tuple[int, int]] = None
    device: Optional[int] = None

    @property
    def host(self) -> str:
        return self.address.rsplit(":", 1)[0]

    @property
    def port(self) -> int:
        return int(self.address.rsplit(":", 1)[-1])


# most alternatives per token that 'logprobs' records: OpenAI's top_logprobs limit; the candidate slots of
# csrc/kernels/logprobs.hip (LP_MAX_N) are sized by it
LOGPROBS_MAX_N = 20


# caps of the stop conditions: the tables of csrc/kernels/stop.hip are sized by them
STOP_MAX_IDS = 16
STOP_MAX_SEQS = 8
STOP_MAX_SEQ_LEN = 16


@dataclass(frozen=True)
class StopConfig:
    """The stop conditions of a generation (runtime/sampling.py ``stop_ref``
    states the semantics): what a last stage gets when any is configured."""

    stop_token_ids: Tuple[int, ...] = ()
    stop_sequences: Tuple[Tuple[int, ...], ...] = ()
    min_new_tokens: int = 0
    pad_token_id: int = 0


def _is_int(v: Any) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def make_stop(vocab: int, eos_token_id: Any = None, stop_token_ids: Any = None, stop_sequences: Any = None,
              min_new_tokens: Any = 0, pad_token_id: Any = None) -> Optional[StopConfig]:
    """Validate the five stop keys against a vocabulary of ``vocab`` entries.
    ``eos_token_id`` (an int or a list of ints) is shorthand: its ids are
    appended to ``stop_token_ids``.  Returns None when there is no stop id and
    no stop sequence (the neutral case); raises ``ConfigError`` otherwise for a
    value out of range, a duplicate, a count above the caps or a
    ``min_new_tokens`` > 0 without anything to stop at."""
    def ids_of(key: str, v: Any) -> List[int]:
        if not isinstance(v, (list, tuple)) or any(not _is_int(e) for e in v):
            raise ConfigError(f"ERROR: '{key}' must be a list of integers, got {v!r}")
        bad = [e for e in v if not 0 <= e < vocab]
        if bad:
            raise ConfigError(f"ERROR: '{key}' holds ids outside [0, {vocab}): {bad!r}")
        return [int(e) for e in v]

    ids = ids_of("stop_token_ids", [] if stop_token_ids is None else stop_token_ids)
    if eos_token_id is not None:
        if isinstance(eos_token_id, bool) or not isinstance(eos_token_id, (int, list, tuple)):
            raise ConfigError(f"ERROR: 'eos_token_id' must be an integer or a list of integers, got {eos_token_id!r}")
        ids += ids_of("eos_token_id", [eos_token_id] if _is_int(eos_token_id) else eos_token_id)
    if len(set(ids)) != len(ids):
        raise ConfigError(f"ERROR: the stop ids ('stop_token_ids' and 'eos_token_id') must be distinct, got {ids!r}")
    if len(ids) > STOP_MAX_IDS:
        raise ConfigError(f"ERROR: at most {STOP_MAX_IDS} stop ids ('stop_token_ids' and 'eos_token_id'), got {len(ids)}")
    seqs_in = [] if stop_sequences is None else stop_sequences
    if not isinstance(seqs_in, (list, tuple)) or any(not isinstance(q, (list, tuple)) for q in seqs_in):
        raise ConfigError(f"ERROR: 'stop_sequences' must be a list of lists of integers, got {stop_sequences!r}")
    if len(seqs_in) > STOP_MAX_SEQS:
        raise ConfigError(f"ERROR: at most {STOP_MAX_SEQS} 'stop_sequences', got {len(seqs_in)}")
    seqs = []
    for q in seqs_in:
        if not 1 <= len(q) <= STOP_MAX_SEQ_LEN:
            raise ConfigError(f"ERROR: every entry of 'stop_sequences' holds 1..{STOP_MAX_SEQ_LEN} ids, got {len(q)}")
        seqs.append(tuple(ids_of("stop_sequences", q)))
    if not _is_int(min_new_tokens) or min_new_tokens < 0:
        raise ConfigError(f"ERROR: 'min_new_tokens' must be an integer >= 0, got {min_new_tokens!r}")
    if pad_token_id is not None and (not _is_int(pad_token_id) or not 0 <= pad_token_id < vocab):
        raise ConfigError(f"ERROR: 'pad_token_id' must be an id in [0, {vocab}), got {pad_token_id!r}")
    if not ids and not seqs:
        if min_new_tokens > 0:
            raise ConfigError("ERROR: 'min_new_tokens' needs at least one stop id or stop sequence "
                              "('eos_token_id', 'stop_token_ids', 'stop_sequences')")
        return None
    pad = int(pad_token_id) if pad_token_id is not None else (ids[0] if ids else 0)
    return StopConfig(tuple(ids), tuple(seqs), int(min_new_tokens), pad)


# caps of the logit constraints: the tables of csrc/kernels/constraints.hip are sized by them
CON_MAX_BIAS = 256
CON_MAX_BAD_WORDS = 64
CON_MAX_BAD_LEN = 16
CON_MAX_NGRAM = 16
CON_MAX_ABS_BIAS = 100.0


@dataclass(frozen=True)
class ConstraintConfig:
    """The hard constraints on the logits of a generation (runtime/sampling.py
    ``constraints_ref`` states the semantics): what a last stage gets when any
    is configured."""

    logit_bias: Tuple[Tuple[int, float], ...] = ()             # (id, bias), distinct ids
    allowed_token_ids: Optional[Tuple[int, ...]] = None        # None = every id is allowed
    bad_words_ids: Tuple[Tuple[int, ...], ...] = ()
    no_repeat_ngram_size: int = 0

    @property
    def needs_context(self) -> bool:
        """Does a rule read the row's ordered context (prompt + generated)?"""
        return self.no_repeat_ngram_size > 0 or any(len(s) > 1 for s in self.bad_words_ids)


def make_constraints(vocab: int, logit_bias: Any = None, allowed_token_ids: Any = None, bad_words_ids: Any = None,
                     no_repeat_ngram_size: Any = 0) -> Optional[ConstraintConfig]:
    """Validate the four constraint keys against a vocabulary of ``vocab``
    entries.  ``logit_bias`` is an object with string or integer keys or a list
    of ``[id, bias]`` pairs.  Returns None when every key is neutral; raises
    ``ConfigError`` for a value out of range, a duplicate, a count above the
    caps, or an ``allowed_token_ids`` whose every member is a one-token bad
    word (nothing could ever be generated)."""
    import math

    def ids_of(key: str, v: Any) -> List[int]:
        if not isinstance(v, (list, tuple)) or any(not _is_int(e) for e in v):
            raise ConfigError(f"ERROR: '{key}' must be a list of integers, got {v!r}")
        bad = [e for e in v if not 0 <= e < vocab]
        if bad:
            raise ConfigError(f"ERROR: '{key}' holds ids outside [0, {vocab}): {bad!r}")
        return [int(e) for e in v]

    bias: List[Tuple[int, float]] = []
    if logit_bias is not None:
        if isinstance(logit_bias, dict):
            pairs = []
            for k, b in logit_bias.items():
                if isinstance(k, str):
                    try:
                        k = int(k.strip())
                    except ValueError:
                        raise ConfigError(f"ERROR: 'logit_bias' key {k!r} is no token id") from None
                pairs.append((k, b))
        elif isinstance(logit_bias, (list, tuple)) and all(isinstance(e, (list, tuple)) and len(e) == 2
                                                           for e in logit_bias):
            pairs = [(e[0], e[1]) for e in logit_bias]
        else:
            raise ConfigError(f"ERROR: 'logit_bias' must be an object {{id: bias}} or a list of [id, bias] pairs, "
                              f"got {logit_bias!r}")
        for k, b in pairs:
            if not _is_int(k) or not 0 <= k < vocab:
                raise ConfigError(f"ERROR: 'logit_bias' id {k!r} outside [0, {vocab})")
            if isinstance(b, bool) or not isinstance(b, (int, float)) or not math.isfinite(b) \
                    or abs(b) > CON_MAX_ABS_BIAS:
                raise ConfigError(f"ERROR: 'logit_bias' of id {k} must be a finite number with |b| <= "
                                  f"{CON_MAX_ABS_BIAS:g}, got {b!r}")
            bias.append((int(k), float(b)))
        if len({k for k, _ in bias}) != len(bias):
            raise ConfigError(f"ERROR: the ids of 'logit_bias' must be distinct, got {[k for k, _ in bias]!r}")
        if len(bias) > CON_MAX_BIAS:
            raise ConfigError(f"ERROR: at most {CON_MAX_BIAS} ids in 'logit_bias', got {len(bias)}")
    allowed = None
    if allowed_token_ids is not None:
        allowed = ids_of("allowed_token_ids", allowed_token_ids)
        if not allowed:
            raise ConfigError("ERROR: 'allowed_token_ids' must not be empty (leave the key out to allow every id)")
        if len(set(allowed)) != len(allowed):
            raise ConfigError("ERROR: the ids of 'allowed_token_ids' must be distinct")
    words_in = [] if bad_words_ids is None else bad_words_ids
    if not isinstance(words_in, (list, tuple)) or any(not isinstance(q, (list, tuple)) for q in words_in):
        raise ConfigError(f"ERROR: 'bad_words_ids' must be a list of lists of integers, got {bad_words_ids!r}")
    if len(words_in) > CON_MAX_BAD_WORDS:
        raise ConfigError(f"ERROR: at most {CON_MAX_BAD_WORDS} 'bad_words_ids', got {len(words_in)}")
    words = []
    for q in words_in:
        if not 1 <= len(q) <= CON_MAX_BAD_LEN:
            raise ConfigError(f"ERROR: every entry of 'bad_words_ids' holds 1..{CON_MAX_BAD_LEN} ids, got {len(q)}")
        words.append(tuple(ids_of("bad_words_ids", q)))
    n = no_repeat_ngram_size
    if not _is_int(n) or not 0 <= n <= CON_MAX_NGRAM:
        raise ConfigError(f"ERROR: 'no_repeat_ngram_size' must be an integer in [0, {CON_MAX_NGRAM}], got {n!r}")
    if allowed is not None and set(allowed) <= {w[0] for w in words if len(w) == 1}:
        raise ConfigError("ERROR: every id of 'allowed_token_ids' is also a one-token entry of 'bad_words_ids': "
                          "nothing could be generated")
    if not bias and allowed is None and not words and n == 0:
        return None
    return ConstraintConfig(tuple(bias), None if allowed is None else tuple(allowed), tuple(words), int(n))


CONSTRAINT_KEYS = ("logit_bias", "allowed_token_ids", "bad_words_ids", "no_repeat_ngram_size")


def make_prompt_lists(vocab: int, prompts: Any, n_seq: int, key: str = "prompts") -> Tuple[Tuple[int, ...], ...]:
    """Validate the prompts of one generation (config key ``prompts``, or the
    parsed ``--prompt``): a list of 1..``n_seq`` non-empty lists of ids in
    ``[0, vocab)``.  Sequence i of the run gets entry ``i % n``, so one prompt
    replicates to every sequence."""
    if (not isinstance(prompts, (list, tuple)) or not prompts
            or any(not isinstance(q, (list, tuple)) or any(not _is_int(e) for e in q) for q in prompts)):
        raise ConfigError(f"ERROR: '{key}' must be a non-empty list of lists of integers, got {prompts!r}")
    if len(prompts) > n_seq:
        raise ConfigError(f"ERROR: '{key}' holds {len(prompts)} prompts, the run has micro_batch_size * "
                          f"num_microbatches = {n_seq} sequences")
    if any(len(q) == 0 for q in prompts):
        raise ConfigError(f"ERROR: '{key}' holds an empty prompt: every prompt needs at least one id")
    bad = [e for q in prompts for e in q if not 0 <= e < vocab]
    if bad:
        raise ConfigError(f"ERROR: '{key}' holds ids outside [0, {vocab}): {bad[:8]!r}")
    return tuple(tuple(int(e) for e in q) for q in prompts)


STOP_KEYS = ("eos_token_id", "stop_token_ids", "stop_sequences", "min_new_tokens", "pad_token_id")


@dataclass
class PipelineConfig:
    """The whole topology: every stage, in stage order."""

    nodes: List[NodeSpec]
    model_weights: str
    num_parts: int
    return_to_node_id: Optional[str] = None
    model: str = "cifar10"
    dtype: Optional[str] = None
    kv_cache_dtype: str = "bf16"              # "fp8": OCP e4m3 KV cache (half the decode K/V bytes)
    kv_cache_scale: str = "calibrated"        # fp8 cache: per-layer scale from the first prefill's amax, or "unit"
    fp8_prefill: str = "e4m3"                 # dtype fp8: prefill activations "e4m3" (one byte, per-row scale) or "split" (e4m3 hi + residual)
    transport: str = "grpc"
    micro_batch_size: int = 1
    num_microbatches: int = 1
    seq_len: int = 64
    prompt_len: Optional[int] = None
    prompts: Optional[Tuple[Tuple[int, ...], ...]] = None  # token ids of 1..n prompts, cycled over the sequences
    decode_steps: int = 0
    prefill_chunk: int = 0                    # > 0: chunked prefill, this many prompt tokens per stage call
    temperature: float = 0.0                  # 0 = greedy; > 0 = sampling (last stage)
    top_k: int = 0                            # 0 = whole vocabulary
    top_p: float = 1.0                        # nucleus: smallest head of the distribution with this mass (1 = off)
    min_p: float = 0.0                        # drop tokens below this fraction of the top probability (0 = off)
    seed: int = 0                             # sampling seed (counter-based RNG, reproducible)
    repetition_penalty: float = 1.0           # > 0; seen (prompt or generated) tokens: logit / r if > 0 else * r (1 = off)
    presence_penalty: float = 0.0             # subtracted once from the logit of every generated token (0 = off)
    frequency_penalty: float = 0.0            # subtracted per time the token was generated (0 = off)
    logprobs: int = 0                         # 1..20: record each token's log-probability and the top-n (0 = off)
    stop: Optional[StopConfig] = None         # stop ids / sequences, min_new_tokens, pad_token_id (None = never stops)
    constraints: Optional[ConstraintConfig] = None  # logit_bias, allowed / bad ids, no_repeat_ngram_size (None = off)
    rpc_timeout_s: Optional[float] = None     # per-hop SendTensor deadline (reference: none)
    health_timeout_s: float = 120.0           # readiness barrier before stage 0 sends
    comm_timeout_s: float = 300.0             # process-group (RCCL/gloo) op timeout
    heartbeat_timeout_s: float = 15.0         # parallel/watchdog.py: peer declared dead after this
    stall_timeout_s: Optional[float] = None   # parallel/watchdog.py: abort when this rank stops progressing
    replicas: int = 1                         # data-parallel copies of the whole pipeline (rccl / gloo)
    input_dtype: str = "fp32"                 # CIFAR stage 0 input: "fp32" (B,3,32,32) or "uint8" (B,32,32,3) images
    input_mean: Tuple[float, float, float] = (0.5, 0.5, 0.5)  # uint8 input: per-channel Normalize mean ...
    input_std: Tuple[float, float, float] = (0.5, 0.5, 0.5)   # ... and std (after the division by 255)
    raw: Dict[str, Any] = field(default_factory=dict)

    def stage(self, part_index: int) -> NodeSpec:
        for n in self.nodes:
            if n.part_index == part_index:
                return n
        raise ConfigError(f"ERROR: Could not find node config for next part index {part_index}")

    def by_id(self, node_id: str) -> Optional[NodeSpec]:
        return next((n for n in self.nodes if n.id == node_id), None)

    @property
    def stages(self) -> List[NodeSpec]:
        return sorted(self.nodes, key=lambda n: n.part_index)


@dataclass
class NodeContext:
    """Per-process view of the config (replaces the reference's module globals,
    ``node.py:17-26``)."""

    node_id: str
    address: str
    port: int
    part_index: int
    num_parts: int
    model_weights: str
    is_last: bool
    next_address: Optional[str]
    return_address: Optional[str]
    pipeline: PipelineConfig
    replica: int = 0  # which data-parallel copy of the pipeline this process serves

    @property
    def node(self) -> NodeSpec:
        return self.pipeline.stage(self.part_index)

    @property
    def rank(self) -> int:
        """Process-group rank: replica-major, ``replica * num_parts + part_index``."""
        return self.replica * self.num_parts + self.part_index

    @property
    def world(self) -> int:
        return self.pipeline.replicas * self.num_parts

    def peer(self, part_index: int) -> int:
        """Rank of stage ``part_index`` of this process's own replica."""
        return self.replica * self.num_parts + part_index


def load_json(path: str) -> Dict[str, Any]:
    """``node.py:222-231``: file-not-found and bad-JSON errors, same wording."""
    try:
        with open(path, "r") as f:
            return json.load(f)
    except FileNotFoundError:
        raise ConfigError(f"ERROR: Config file not found at '{path}'")
    except json.JSONDecodeError as e:
        raise ConfigError(f"ERROR: Invalid JSON in config file '{path}': {e}")


def _parse_layers(v: Any) -> Optional[Tuple[int, int]]:
    if v is None:
        return None
    if not (isinstance(v, (list, tuple)) and len(v) == 2 and all(isinstance(i, int) for i in v)):
        raise ConfigError(f"ERROR: 'layers' must be [start, end] (inclusive), got {v!r}")
    if v[0] > v[1] or v[0] < 0:
        raise ConfigError(f"ERROR: invalid layer range {v!r}")
    return (int(v[0]), int(v[1]))


def parse_pipeline(cfg: Dict[str, Any], path: str = "<config>") -> PipelineConfig:
    raw_nodes = cfg.get("nodes", [])
    num_parts = cfg.get("num_parts")
    weights = cfg.get("model_weights")
    nodes: List[NodeSpec] = []
    for n in raw_nodes:
        if n.get("address") is None or n.get("part_index") is None:
            raise ConfigError("ERROR: Config file is missing required fields (address, part_index, model_weights, num_parts)")
        address = n["address"]
        try:
            int(str(address).split(":")[-1])
        except (ValueError, IndexError):
            raise ConfigError(f"ERROR: Invalid format for MY_ADDRESS '{address}'. Expected IP:Port.")
        nodes.append(NodeSpec(id=str(n.get("id")), address=str(address), part_index=int(n["part_index"]),
                              layers=_parse_layers(n.get("layers")), device=n.get("device")))
    if None in [weights, num_parts]:
        raise ConfigError("ERROR: Config file is missing required fields (address, part_index, model_weights, num_parts)")
    if not isinstance(num_parts, int) or num_parts < 1:
        raise ConfigError(f"ERROR: Configuration file specifies num_parts={num_parts}, but this script expects a positive integer.")
    idx = sorted(n.part_index for n in nodes)
    if idx != list(range(num_parts)):
        raise ConfigError(f"ERROR: Configuration file specifies num_parts={num_parts}, but part_index values are {idx}; "
                          f"expected a permutation of 0..{num_parts - 1}.")
    transport = cfg.get("transport", "grpc")
    if transport not in TRANSPORTS:
        raise ConfigError(f"ERROR: unknown transport '{transport}', expected one of {TRANSPORTS}")
    model = cfg.get("model", "cifar10")
    if model not in MODELS:
        raise ConfigError(f"ERROR: unknown model '{model}', expected one of {MODELS}")
    for key in ("micro_batch_size", "num_microbatches"):
        v = cfg.get(key, 1)
        if not isinstance(v, int) or v < 1:
            raise ConfigError(f"ERROR: '{key}' must be a positive integer, got {v!r}")
    for key in ("prefill_chunk", "decode_steps", "top_k", "seed"):
        v = cfg.get(key, 0)
        if not isinstance(v, int) or isinstance(v, bool) or v < 0:
            raise ConfigError(f"ERROR: '{key}' must be a non-negative integer, got {v!r}")
    for key in ("heartbeat_timeout_s", "stall_timeout_s", "health_timeout_s", "comm_timeout_s", "rpc_timeout_s"):
        v = cfg.get(key)
        if v is not None and (not isinstance(v, (int, float)) or isinstance(v, bool) or v <= 0):
            raise ConfigError(f"ERROR: '{key}' must be a positive number of seconds, got {v!r}")
    reps = cfg.get("replicas", 1)
    if not isinstance(reps, int) or isinstance(reps, bool) or reps < 1:
        raise ConfigError(f"ERROR: 'replicas' must be a positive integer, got {reps!r}")
    if reps > 1 and transport not in DIST_TRANSPORTS:
        raise ConfigError(f"ERROR: 'replicas' > 1 needs transport 'rccl', 'gloo' or 'gloo_gpu' (one rank per stage and replica), "
                          f"got '{transport}'")
    kvd = cfg.get("kv_cache_dtype", "bf16")
    if kvd not in ("bf16", "fp8"):
        raise ConfigError(f"ERROR: 'kv_cache_dtype' must be 'bf16' or 'fp8', got {kvd!r}")
    fpp = cfg.get("fp8_prefill", "e4m3")
    if fpp not in ("split", "e4m3"):
        raise ConfigError(f"ERROR: 'fp8_prefill' must be 'split' or 'e4m3', got {fpp!r}")
    kvs = cfg.get("kv_cache_scale", "calibrated")
    if kvs not in ("calibrated", "unit"):
        raise ConfigError(f"ERROR: 'kv_cache_scale' must be 'calibrated' or 'unit', got {kvs!r}")
    t = cfg.get("temperature", 0.0)
    if not isinstance(t, (int, float)) or t < 0:
        raise ConfigError(f"ERROR: 'temperature' must be >= 0, got {t!r}")
    tp = cfg.get("top_p", 1.0)
    if not isinstance(tp, (int, float)) or isinstance(tp, bool) or not 0 < tp <= 1:
        raise ConfigError(f"ERROR: 'top_p' must be in (0, 1], got {tp!r}")
    mp = cfg.get("min_p", 0.0)
    if not isinstance(mp, (int, float)) or isinstance(mp, bool) or not 0 <= mp < 1:
        raise ConfigError(f"ERROR: 'min_p' must be in [0, 1), got {mp!r}")
    rp = cfg.get("repetition_penalty", 1.0)
    if not isinstance(rp, (int, float)) or isinstance(rp, bool) or not (rp > 0 and math.isfinite(rp)):
        raise ConfigError(f"ERROR: 'repetition_penalty' must be a finite number > 0, got {rp!r}")
    pens = {}
    for key in ("presence_penalty", "frequency_penalty"):
        v = cfg.get(key, 0.0)
        if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v):
            raise ConfigError(f"ERROR: '{key}' must be a finite number, got {v!r}")
        pens[key] = float(v)
    nlp = cfg.get("logprobs", 0)
    if not isinstance(nlp, int) or isinstance(nlp, bool) or not 0 <= nlp <= LOGPROBS_MAX_N:
        raise ConfigError(f"ERROR: 'logprobs' must be an integer in [0, {LOGPROBS_MAX_N}], got {nlp!r}")
    if model == "cifar10" and nlp != 0:
        raise ConfigError(f"ERROR: 'logprobs' {nlp!r} exists for the generating models only, got model '{model}'")
    stop = None
    if any(cfg.get(k) is not None for k in STOP_KEYS):
        if model == "cifar10":
            raise ConfigError(f"ERROR: {[k for k in STOP_KEYS if cfg.get(k) is not None]!r} exist for the generating "
                              f"models only, got model '{model}'")
        from .models import model_info  # the vocabulary (imports torch: only when a stop key is present)
        stop = make_stop(model_info(model).cfg.vocab_size, **{k: cfg.get(k) for k in STOP_KEYS if k != "min_new_tokens"},
                         min_new_tokens=cfg.get("min_new_tokens", 0))
    cons = None
    if any(cfg.get(k) is not None for k in CONSTRAINT_KEYS):
        if model == "cifar10":
            raise ConfigError(f"ERROR: {[k for k in CONSTRAINT_KEYS if cfg.get(k) is not None]!r} exist for the "
                              f"generating models only, got model '{model}'")
        from .models import model_info  # the vocabulary (imports torch: only when a constraint key is present)
        cons = make_constraints(model_info(model).cfg.vocab_size,
                                **{k: cfg.get(k) for k in CONSTRAINT_KEYS if k != "no_repeat_ngram_size"},
                                no_repeat_ngram_size=cfg.get("no_repeat_ngram_size", 0))
    if model == "cifar10":
        for key, v, neutral in (("repetition_penalty", rp, 1), ("presence_penalty", pens["presence_penalty"], 0),
                                ("frequency_penalty", pens["frequency_penalty"], 0)):
            if v != neutral:
                raise ConfigError(f"ERROR: '{key}' {v!r} exists for the generating models only, got model '{model}'")
    prompts = None
    if cfg.get("prompts") is not None:
        if model == "cifar10":
            raise ConfigError(f"ERROR: 'prompts' exists for the generating models only, got model '{model}'")
        from .models import model_info  # the vocabulary (imports torch: only when the key is present)
        prompts = make_prompt_lists(model_info(model).cfg.vocab_size, cfg.get("prompts"),
                                    int(cfg.get("micro_batch_size", 1)) * int(cfg.get("num_microbatches", 1)))
    idt = cfg.get("input_dtype", "fp32")
    if idt not in ("fp32", "uint8"):
        raise ConfigError(f"ERROR: 'input_dtype' must be 'fp32' or 'uint8', got {idt!r}")
    if idt == "uint8" and model != "cifar10":
        raise ConfigError(f"ERROR: 'input_dtype' 'uint8' exists for model 'cifar10' only, got model '{model}'")
    norm = {}
    for key in ("input_mean", "input_std"):
        v = cfg.get(key, [0.5, 0.5, 0.5])
        if (not isinstance(v, (list, tuple)) or len(v) != 3
                or any(not isinstance(e, (int, float)) or isinstance(e, bool) for e in v)):
            raise ConfigError(f"ERROR: '{key}' must be three numbers (one per channel), got {v!r}")
        norm[key] = tuple(float(e) for e in v)
    if any(e == 0 for e in norm["input_std"]):
        raise ConfigError(f"ERROR: 'input_std' must be nonzero in every channel, got {cfg.get('input_std')!r}")
    ret = cfg.get("return_to_node_id")
    if ret is not None and transport in DIST_TRANSPORTS:
        rn = next((n for n in nodes if n.id == ret), None)
        if rn is None:
            raise ConfigError(f"ERROR: return_to_node_id '{ret}' is not a node of this config")
    return PipelineConfig(
        nodes=nodes, model_weights=str(weights), num_parts=num_parts,
        return_to_node_id=cfg.get("return_to_node_id"), model=model, dtype=cfg.get("dtype"), kv_cache_dtype=kvd,
        kv_cache_scale=kvs, fp8_prefill=fpp,
        transport=transport, micro_batch_size=int(cfg.get("micro_batch_size", 1)),
        num_microbatches=int(cfg.get("num_microbatches", 1)), seq_len=int(cfg.get("seq_len", 64)),
        prompt_len=cfg.get("prompt_len"), prompts=prompts, decode_steps=int(cfg.get("decode_steps", 0)),
        prefill_chunk=int(cfg.get("prefill_chunk", 0)),
        temperature=float(cfg.get("temperature", 0.0)), top_k=int(cfg.get("top_k", 0)), seed=int(cfg.get("seed", 0)),
        top_p=float(tp), min_p=float(mp), repetition_penalty=float(rp), presence_penalty=pens["presence_penalty"],
        frequency_penalty=pens["frequency_penalty"], logprobs=nlp, stop=stop, constraints=cons,
        rpc_timeout_s=cfg.get("rpc_timeout_s"), health_timeout_s=float(cfg.get("health_timeout_s", 120.0)),
        comm_timeout_s=float(cfg.get("comm_timeout_s", 300.0)),
        heartbeat_timeout_s=float(cfg.get("heartbeat_timeout_s", 15.0)),
        stall_timeout_s=(None if cfg.get("stall_timeout_s") is None else float(cfg["stall_timeout_s"])),
        replicas=int(reps), input_dtype=idt, input_mean=norm["input_mean"], input_std=norm["input_std"], raw=cfg)


def resolve_node(cfg: Dict[str, Any], node_id: str, path: str = "<config>", replica: int = 0) -> NodeContext:
    """Own-node lookup + topology (``node.py:234-278``); ``replica`` selects the
    data-parallel copy of the pipeline (config ``replicas``)."""
    mine = next((n for n in cfg.get("nodes", []) if n.get("id") == node_id), None)
    if not mine:
        raise ConfigError(f"ERROR: Node ID '{node_id}' not found in config file '{path}'")
    address, part_index = mine.get("address"), mine.get("part_index")
    if None in [address, part_index, cfg.get("model_weights"), cfg.get("num_parts")]:
        raise ConfigError("ERROR: Config file is missing required fields (address, part_index, model_weights, num_parts)")
    try:
        port = int(str(address).split(":")[-1])
    except (ValueError, IndexError):
        raise ConfigError(f"ERROR: Invalid format for MY_ADDRESS '{address}'. Expected IP:Port.")
    pipe = parse_pipeline(cfg, path)
    is_last = part_index == pipe.num_parts - 1
    next_address = None
    return_address = None
    if not is_last:
        nxt = next((n for n in pipe.nodes if n.part_index == part_index + 1), None)
        if nxt is None:
            raise ConfigError(f"ERROR: Could not find node config for next part index {part_index + 1}")
        if not nxt.address:
            raise ConfigError(f"ERROR: Next node (index {part_index + 1}) is missing address in config")
        next_address = nxt.address
    else:
        # The reference resolves this and never uses it (node.py:272-277); here it is
        # the ring back-edge: where the last stage sends results / sampled tokens.
        if pipe.return_to_node_id:
            ret = pipe.by_id(pipe.return_to_node_id)
            if ret is not None:
                return_address = ret.address
    if not (isinstance(replica, int) and 0 <= replica < pipe.replicas):
        raise ConfigError(f"ERROR: replica {replica!r} out of range: the config has {pipe.replicas} replica(s)")
    return NodeContext(node_id=node_id, address=str(address), port=port, part_index=int(part_index),
                       num_parts=pipe.num_parts, model_weights=pipe.model_weights, is_last=is_last,
                       next_address=next_address, return_address=return_address, pipeline=pipe, replica=replica)


def load_node(path: str, node_id: str, replica: int = 0) -> NodeContext:
    return resolve_node(load_json(path), node_id, path, replica)


def banner(ctx: NodeContext, device: str) -> str:
    """Config banner (``node.py:280-290``), same lines."""
    return "\n".join([
        "--- Node Configuration ---",
        f"  ID: {ctx.node_id}",
        f"  Full Address (for clients): {ctx.address}",
        f"  Server Listening Port: {ctx.port}",
        f"  Part Index: {ctx.part_index} / {ctx.num_parts - 1}",
        f"  Is Last: {ctx.is_last}",
        f"  Next Node Address: {ctx.next_address}",
        f"  Return Node Addr: {ctx.return_address}",
        f"  Weights: {ctx.model_weights}",
        f"  Device: {device}",
        f"  Model: {ctx.pipeline.model}  Transport: {ctx.pipeline.transport}"
        + (f"  Replica: {ctx.replica} / {ctx.pipeline.replicas - 1}" if ctx.pipeline.replicas > 1 else ""),
        "-------------------------",
    ])
