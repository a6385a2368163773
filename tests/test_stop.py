"""Stop tokens, stop sequences and min_new_tokens on the CPU: the config keys,
the torch mirror (runtime/sampling.py stop_ref) against a plain Python loop,
the named edge cases, TorchStage rings against the unstopped run with the
mirror applied on the host, and two gloo ranks against one process."""
import json
import os
import subprocess
import sys

import pytest
import torch

from distributed_neural_networks_amd.runtime.sampling import STOP_STATE_WORDS, stop_reason, stop_ref, stop_state, \
    stop_suppress_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, PYTHONPATH=ROOT, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")


# ---------------------------------------------------------------------- the third implementation: a plain loop
def loop_ref(stream, ids, seqs, min_new, pad):
    """One row.  ``stream``: the tokens the sampler picks, step by step (what it
    would pick for a finished row does not matter: any value may stand there).
    Returns (output tokens, finish length or 0, reason or None)."""
    out, gen, fin = [], [], None
    for t in stream:
        if fin is not None:
            out.append(pad)
            continue
        gen.append(t)
        out.append(t)
        g = len(gen)
        if t in ids:
            fin = (g, ("token", list(ids).index(t)))
            continue
        for k, s in enumerate(seqs):
            if g >= max(min_new, len(s)) and gen[-len(s):] == list(s):
                fin = (g, ("sequence", k))
                break
    return out, (fin[0] if fin else 0), (fin[1] if fin else None)


def run_mirror(streams, ids, seqs, min_new, pad):
    """``stop_ref`` step by step over (M, steps) streams: (padded tokens, final state)."""
    streams = torch.as_tensor(streams, dtype=torch.int32)
    st = stop_state(streams.shape[0])
    cols = []
    for j in range(streams.shape[1]):
        before = (st.clone(), streams[:, j].clone())
        st, t = stop_ref(st, streams[:, j], ids, seqs, min_new, pad)
        assert torch.equal(before[0][:, 0] + (before[0][:, 1] == 0).int(), st[:, 0])  # g counts running rows only
        assert t.dtype == torch.int32 and st.dtype == torch.int32 and st.shape == (streams.shape[0], STOP_STATE_WORDS)
        cols.append(t)
    return torch.stack(cols, 1), st


def check_against_loop(streams, ids, seqs, min_new, pad):
    toks, st = run_mirror(streams, ids, seqs, min_new, pad)
    for r, row in enumerate(torch.as_tensor(streams).tolist()):
        out, length, reason = loop_ref(row, ids, seqs, min_new, pad)
        assert toks[r].tolist() == out, (r, row, toks[r].tolist(), out)
        assert int(st[r, 1]) == length and stop_reason(st[r, 2]) == reason, (r, row, st[r].tolist(), length, reason)
    return toks, st


# ---------------------------------------------------------------------- config
def _cfg(**kw):
    d = {"nodes": [{"id": "a", "address": "127.0.0.1:1", "part_index": 0}], "model_weights": "synthetic:0",
         "num_parts": 1, "model": "gpt2-tiny"}
    d.update(kw)
    return d


def test_config_keys():
    from distributed_neural_networks_amd.config import ConfigError, StopConfig, load_json, parse_pipeline
    from distributed_neural_networks_amd.models import model_info
    V = model_info("gpt2-tiny").cfg.vocab_size
    assert parse_pipeline(_cfg()).stop is None
    assert parse_pipeline(_cfg(min_new_tokens=0, stop_token_ids=[], stop_sequences=[])).stop is None  # neutral
    # eos_token_id: an int or a list, appended to stop_token_ids
    assert parse_pipeline(_cfg(eos_token_id=7)).stop == StopConfig((7,), (), 0, 7)
    assert parse_pipeline(_cfg(eos_token_id=[7, 9])).stop == StopConfig((7, 9), (), 0, 7)
    p = parse_pipeline(_cfg(stop_token_ids=[3, 4], eos_token_id=[7], stop_sequences=[[1, 2], [5]], min_new_tokens=6))
    assert p.stop == StopConfig((3, 4, 7), ((1, 2), (5,)), 6, 3)
    # pad_token_id: the first stop id, 0 without one, or the key
    assert parse_pipeline(_cfg(stop_sequences=[[1, 2]])).stop.pad_token_id == 0
    assert parse_pipeline(_cfg(stop_sequences=[[1, 2]], pad_token_id=V - 1)).stop.pad_token_id == V - 1
    assert parse_pipeline(_cfg(eos_token_id=5, pad_token_id=5)).stop.pad_token_id == 5
    # ranges
    for bad in ([-1], [V], [1.5], ["2"], [True], 3, "x"):
        with pytest.raises(ConfigError, match="stop_token_ids"):
            parse_pipeline(_cfg(stop_token_ids=bad))
    for bad in (-1, V, 1.5, "2", True, [V], [[1]]):
        with pytest.raises(ConfigError, match="eos_token_id"):
            parse_pipeline(_cfg(eos_token_id=bad))
    for bad in ([[]], [list(range(17))], [[V]], [[-1]], [3], [[1.5]], 7, [[0]] * 9):
        with pytest.raises(ConfigError, match="stop_sequences"):
            parse_pipeline(_cfg(stop_sequences=bad))
    for bad in (-1, V, 2.5, True):
        with pytest.raises(ConfigError, match="pad_token_id"):
            parse_pipeline(_cfg(eos_token_id=1, pad_token_id=bad))
    for bad in (-1, 2.5, True, "1"):
        with pytest.raises(ConfigError, match="min_new_tokens"):
            parse_pipeline(_cfg(eos_token_id=1, min_new_tokens=bad))
    # caps: 16 ids (eos included), 8 sequences of at most 16
    assert len(parse_pipeline(_cfg(stop_token_ids=list(range(15)), eos_token_id=15)).stop.stop_token_ids) == 16
    with pytest.raises(ConfigError, match="at most 16 stop ids"):
        parse_pipeline(_cfg(stop_token_ids=list(range(16)), eos_token_id=16))
    assert len(parse_pipeline(_cfg(stop_sequences=[list(range(16))] * 8)).stop.stop_sequences) == 8
    # duplicates, also across the two keys
    with pytest.raises(ConfigError, match="distinct"):
        parse_pipeline(_cfg(stop_token_ids=[4, 4]))
    with pytest.raises(ConfigError, match="distinct"):
        parse_pipeline(_cfg(stop_token_ids=[4], eos_token_id=4))
    # min_new_tokens needs something to stop at
    with pytest.raises(ConfigError, match="needs at least one stop id or stop sequence"):
        parse_pipeline(_cfg(min_new_tokens=3))
    with pytest.raises(ConfigError, match="generating models only"):
        parse_pipeline(_cfg(model="cifar10", eos_token_id=3))
    path = os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_stop.json")
    p = parse_pipeline(load_json(path), path)
    assert p.stop == StopConfig((0, 50256), ((198, 198), (13, 198)), 4, 0)
    q = parse_pipeline(load_json(os.path.join(ROOT, "configs", "gpt2_4stage_1gpu_sampled.json")))
    assert q.stop is None
    for key in ("temperature", "top_k", "top_p", "seed", "model", "num_parts", "micro_batch_size"):
        assert getattr(p, key) == getattr(q, key)  # the sampled config plus the stop keys


# ---------------------------------------------------------------------- mirror against the loop
@pytest.mark.parametrize("ids,seqs,min_new", [
    ((), (), 0),
    ((3,), (), 0),
    ((), ((0, 1),), 0),
    ((3, 2), ((0, 1), (1, 1, 0), (1,)), 0),
    ((), ((0, 1, 0), (0, 1), (1, 0, 1, 0)), 0),  # shared prefixes and suffixes
    ((3,), ((0, 1), (2, 2, 2)), 5),
    ((), ((0,), (1, 2)), 9),
    ((), ((0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 2, 0), (1, 0)), 0),
], ids=lambda v: str(v).replace(" ", ""))
def test_mirror_against_plain_loop(ids, seqs, min_new):
    g = torch.Generator().manual_seed(11 + len(ids) + 3 * len(seqs) + min_new)
    streams = torch.randint(0, 4, (96, 24), generator=g)
    streams[:8] = torch.tensor([0, 1, 2] * 8)  # the period of the 16-token sequence
    toks, st = check_against_loop(streams, ids, seqs, min_new, pad=1)
    if ids or seqs:
        n_fin = int((st[:, 1] != 0).sum())
        assert 0 < n_fin  # over this alphabet matches are frequent: the comparison is not vacuous
    else:
        assert torch.equal(toks, streams.int()) and int(st[:, 1].abs().sum()) == 0 and bool((st[:, 0] == 24).all())


# ---------------------------------------------------------------------- named cases
def test_overlapping_sequence_stops_at_its_first_completion():
    toks, st = check_against_loop([[5, 5, 5]], (), ((5, 5),), 0, pad=9)
    assert toks.tolist() == [[5, 5, 9]] and st[0, :3].tolist() == [2, 2, 17]


def test_sixteen_token_sequence():
    """It cannot match before token 16, and the -1 entries of a young window
    never stand in for tokens (no id is negative, and g >= len guards it)."""
    seq = tuple([7] * 16)
    toks, st = check_against_loop([[7] * 20], (), (seq,), 0, pad=0)
    assert int(st[0, 1]) == 16 and toks[0].tolist() == [7] * 16 + [0] * 4
    # 15 matching tokens are not enough, whatever came before them
    toks, st = check_against_loop([[3] + [7] * 15 + [3, 3]], (), (seq,), 0, pad=0)
    assert int(st[0, 1]) == 0
    mixed = tuple(range(20, 36))
    stream = [1, 2] + list(mixed) + [4]
    toks, st = check_against_loop([stream, [2, 1] + list(mixed[1:]) + [4, 4]], (), (mixed,), 0, pad=0)
    assert st[:, 1].tolist() == [18, 0] and toks[0].tolist() == stream[:18] + [0]


def test_first_token_takes_part():
    """Token 1 is the one sampled from the prompt's last position."""
    toks, st = check_against_loop([[4, 6, 1], [6, 1, 1]], (), ((4, 6),), 0, pad=0)
    assert st[:, 1].tolist() == [2, 0]
    toks, st = check_against_loop([[4, 6, 1]], (4,), (), 0, pad=2)
    assert st[0, :3].tolist() == [1, 1, 1] and toks.tolist() == [[4, 2, 2]]


def test_stop_id_wins_and_lowest_index_wins():
    # token 6 completes the sequences (4, 6) and (6,) and is stop id number 1
    toks, st = check_against_loop([[4, 6, 0]], (9, 6), ((4, 6), (6,)), 0, pad=0)
    assert stop_reason(st[0, 2]) == ("token", 1) and int(st[0, 1]) == 2
    toks, st = check_against_loop([[4, 6, 0]], (9,), ((5, 6), (4, 6), (6,)), 0, pad=0)
    assert stop_reason(st[0, 2]) == ("sequence", 1)
    toks, st = check_against_loop([[4, 6, 0]], (), ((6,), (4, 6)), 0, pad=0)
    assert stop_reason(st[0, 2]) == ("sequence", 0)


def test_finished_row_never_retriggers():
    """Pad tokens equal to a stop id, and picks that would complete a sequence,
    change nothing after the finish: record, g and window stay."""
    toks, st1 = run_mirror([[1, 3]], (3, 1), ((1, 1),), 0, pad=1)
    st = st1
    for t in (1, 1, 3, 1):
        st, out = stop_ref(st, torch.tensor([t]), (3, 1), ((1, 1),), 0, 1)
        assert out.tolist() == [1] and torch.equal(st, st1)
    assert st1[0, :3].tolist() == [1, 1, 2]  # finished at token 1 by stop id number 1
    check_against_loop([[2, 3, 3, 1, 1, 3]], (3,), ((1, 1),), 0, pad=3)


def test_min_new_tokens_delays_both_kinds():
    # sequences: a completion before min_new does not count, a later one does
    toks, st = check_against_loop([[4, 6, 4, 6, 4, 6, 2]], (), ((4, 6),), 5, pad=0)
    assert st[0, :3].tolist() == [6, 6, 17]
    toks, st = check_against_loop([[4, 6, 2, 2, 2, 2, 2]], (), ((4, 6),), 5, pad=0)
    assert int(st[0, 1]) == 0
    # stop ids: suppression keeps them from being picked while g < min_new (the rows' state decides)
    x = torch.zeros((3, 8))
    x[:, 5], x[:, 2] = 4.0, 3.0
    st = stop_state(3)
    st[0, 0], st[1, 0], st[2, 0] = 1, 2, 0
    st[2, 1], st[2, 2] = 1, 1  # finished: left alone
    y = stop_suppress_ref(x, st, (5, 2), 2)
    assert y[0, 5] == float("-inf") and y[0, 2] == float("-inf") and \
        torch.equal(y[0, [0, 1, 3, 4, 6, 7]], x[0, [0, 1, 3, 4, 6, 7]])
    assert torch.equal(y[1:], x[1:]) and float(x[0, 5]) == 4.0  # g = min_new: no longer; the input is not changed
    assert torch.equal(stop_suppress_ref(x, st, (5, 2), 0), x) and torch.equal(stop_suppress_ref(x, st, (), 3), x)
    assert int(y[0].argmax()) not in (5, 2)


def test_pad_equal_to_a_stop_id():
    toks, st = check_against_loop([[2, 7, 5, 7], [7, 7, 7, 7], [1, 2, 3, 4]], (7,), (), 0, pad=7)
    assert toks.tolist() == [[2, 7, 7, 7], [7, 7, 7, 7], [1, 2, 3, 4]] and st[:, 1].tolist() == [2, 1, 0]


# ---------------------------------------------------------------------- TorchStage rings
def _tiny(seed=5):
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.models import model_info
    model = "gpt2-tiny"
    n = model_info(model).num_layers
    sd = ckpt.random_stage_state_dict(model, 0, n - 1, True, True, seed)
    return model, n, sd, model_info(model).cfg.vocab_size


def _prompts(V, Mb, B, T, seed=4):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, V, (B, T), generator=g) for _ in range(Mb)]


def choose_stops(ref):
    """From an unstopped run's (rows, steps) tokens: one stop id and one
    2-token stop sequence (a row's tokens 1 and 2: the prefill's token takes
    part) such that, by the plain loop, at least one row stops midway on the
    id, at least one on the sequence and at least one never.  Returns
    (ids, seqs, lengths, reasons)."""
    rows, steps = ref.shape
    data = ref.tolist()
    for r in range(rows):
        for j in range(2, steps - 2):
            ids = (data[r][j],)
            for q in range(rows):
                seqs = (tuple(data[q][:2]),)
                res = [loop_ref(row, ids, seqs, 0, 0) for row in data]
                lens, why = [x[1] for x in res], [x[2] for x in res]
                if (any(w == ("token", 0) and 2 < n < steps for n, w in zip(lens, why))
                        and any(w == ("sequence", 0) for w in why) and any(w is None for w in why)):
                    return ids, seqs, lens, why
    raise AssertionError(f"no stop id / sequence with the wanted outcome in {data}")


def expected_from(ref, stop):
    """The unstopped run with the mirror applied on the host."""
    toks, st = run_mirror(ref, stop.stop_token_ids, stop.stop_sequences, stop.min_new_tokens, stop.pad_token_id)
    length = torch.where(st[:, 1] != 0, st[:, 1], torch.tensor(ref.shape[1], dtype=torch.int32))
    return toks, length.int(), [stop_reason(c) for c in st[:, 2].tolist()]


@pytest.fixture(scope="module")
def greedy_ref():
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    model, n, sd, V = _tiny()
    Mb, B, T, steps = 2, 3, 8, 12
    prompts = _prompts(V, Mb, B, T)
    ring = DecodeRing([TorchStage(model, sd, 0, n - 1, True, True, sampling=(0.0, 0, 0))], RingLinks(), 1, Mb, B,
                      use_graphs=False)
    ref = ring.generate(prompts, T, steps).clone()
    with pytest.raises(ValueError, match="no stop conditions"):
        ring.finished()
    return model, n, sd, V, Mb, B, T, steps, prompts, ref


def _stage(model, sd, n, stop, sampling=(0.0, 0, 0, 1.0, 0.0)):
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    return TorchStage(model, sd, 0, n - 1, True, True, sampling=sampling + (1.0, 0.0, 0.0, 0, stop))


def test_torch_stage_ring_equals_unstopped_run_with_mirror(greedy_ref):
    """No operation of a decode step mixes batch rows and the shapes are the
    same in both runs, so a running row's tokens are those of the unstopped
    run, bit for bit, whatever the finished rows are fed."""
    from distributed_neural_networks_amd.config import StopConfig
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    model, n, sd, V, Mb, B, T, steps, prompts, ref = greedy_ref
    ids, seqs, lens, why = choose_stops(ref)
    # the facts the choice rests on, on the reference run itself
    assert any(w == ("token", 0) and 2 < k < steps for k, w in zip(lens, why)) and any(w is None for w in why)
    assert any(w == ("sequence", 0) and k == 2 for k, w in zip(lens, why))  # tokens 1 and 2: the prefill's takes part
    pad = (ids[0] + 1) % V
    stop = StopConfig(ids, seqs, 0, pad)
    want_t, want_len, want_why = expected_from(ref, stop)
    st = _stage(model, sd, n, stop)
    ring = DecodeRing([st], RingLinks(), 1, Mb, B, use_graphs=False, early_exit=False)
    toks = ring.generate(prompts, T, steps)
    fin = ring.finished()
    assert torch.equal(toks, want_t), (toks.tolist(), want_t.tolist())
    assert torch.equal(fin["length"], want_len) and fin["length"].dtype == torch.int32 and fin["reason"] == want_why
    for r in range(Mb * B):  # padded past the length, the stop token / sequence kept
        assert toks[r, int(want_len[r]):].tolist() == [pad] * (steps - int(want_len[r]))
        assert toks[r, :int(want_len[r])].tolist() == ref[r, :int(want_len[r])].tolist()
    # chunked prefill (the discarded samples of the first pieces are forgotten) equals unchunked
    ring_c = DecodeRing([_stage(model, sd, n, stop)], RingLinks(), 1, Mb, B, use_graphs=False, early_exit=False)
    assert torch.equal(ring_c.generate(prompts, T, steps, chunk=3), toks)
    fc = ring_c.finished()
    assert torch.equal(fc["length"], want_len) and fc["reason"] == want_why
    # a second generation on the same ring repeats the first
    assert torch.equal(ring.generate(prompts, T, steps), toks)
    f2 = ring.finished()
    assert torch.equal(f2["length"], want_len) and f2["reason"] == want_why
    # a shorter one reports the tokens generated so far for the rows that never stopped
    short = ring.generate(prompts, T, 5)
    assert torch.equal(short, want_t[:, :5])
    assert torch.equal(ring.finished()["length"], torch.where(want_len <= 5, want_len, torch.tensor(5, dtype=torch.int32)))


def test_chunked_prefill_forgets_the_discarded_samples(greedy_ref):
    """Every prefill piece samples a token; only the last piece's is token 1.
    With the stop id set to what a first piece samples, forgetting matters."""
    from distributed_neural_networks_amd.config import StopConfig
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    model, n, sd, V, Mb, B, T, steps, prompts, ref = greedy_ref
    # what the first piece (3 tokens) of microbatch 0 samples for its row 0
    probe = DecodeRing([_stage(model, sd, n, None)], RingLinks(), 1, 1, B, use_graphs=False)
    first = int(probe.generate([prompts[0][:, :3]], 3, 1)[0, 0])
    stop = StopConfig((first,), (), 0, 0)
    want_t, want_len, want_why = expected_from(ref, stop)
    ring = DecodeRing([_stage(model, sd, n, stop)], RingLinks(), 1, Mb, B, use_graphs=False, early_exit=False)
    assert torch.equal(ring.generate(prompts, T, steps, chunk=3), want_t)
    assert torch.equal(ring.finished()["length"], want_len)


def test_sampled_ring_with_min_new_tokens():
    """Sampled decoding with min_new_tokens: the unstopped run cannot be the
    reference (suppression changes the logits), so the stopped run is checked
    against its own definition: no stop id before the threshold, the finish
    record equal to the plain loop over the run's own tokens."""
    from distributed_neural_networks_amd.config import StopConfig
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    model, n, sd, V = _tiny()
    Mb, B, T, steps, min_new = 2, 3, 8, 12, 6
    prompts = _prompts(V, Mb, B, T)
    samp = (0.9, 0, 3, 1.0, 0.0)
    free = DecodeRing([_stage(model, sd, n, None, samp)], RingLinks(), 1, Mb, B, use_graphs=False).generate(
        prompts, T, steps)
    ids = tuple(sorted(set(free[:, :3].flatten().tolist())))[:16]  # ids the free run picks early
    assert bool(torch.isin(free[:, :min_new], torch.tensor(ids)).any())
    stop = StopConfig(ids, (), min_new, 0)
    ring = DecodeRing([_stage(model, sd, n, stop, samp)], RingLinks(), 1, Mb, B, use_graphs=False, early_exit=False)
    toks = ring.generate(prompts, T, steps)
    assert not bool(torch.isin(toks[:, :min_new], torch.tensor(ids)).any())
    fin = ring.finished()
    for r, row in enumerate(toks.tolist()):
        k = int(fin["length"][r])
        out, length, why = loop_ref(row[:k], ids, (), min_new, 0)
        assert (length or steps) == k and why == fin["reason"][r] and row[k:] == [0] * (steps - k)
        assert k > min_new or why is None


def test_early_exit_on_the_cpu(greedy_ref):
    from distributed_neural_networks_amd.config import StopConfig
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    model, n, sd, V, Mb, B, T, steps, prompts, ref = greedy_ref
    ids = tuple(sorted(set(ref[:, 2].tolist())))  # every row stops by token 3
    stop = StopConfig(ids, (), 0, 0)
    full = DecodeRing([_stage(model, sd, n, stop)], RingLinks(), 1, Mb, B, use_graphs=False, early_exit=False)
    want = full.generate(prompts, T, 30)
    assert int(full.finished()["length"].max()) <= 3 and want.shape[1] == 30
    ring = DecodeRing([_stage(model, sd, n, stop)], RingLinks(), 1, Mb, B, use_graphs=False, multi_step=4)
    assert ring.early_exit
    toks = ring.generate(prompts, T, 30)
    assert toks.shape[1] < 30 and toks.shape[1] <= 3 + 2 * 4
    assert torch.equal(toks, want[:, :toks.shape[1]])
    assert torch.equal(ring.finished()["length"], full.finished()["length"])
    # a ring whose rows never all stop runs every round
    assert not DecodeRing([_stage(model, sd, n, None)], RingLinks(), 1, Mb, B, use_graphs=False).early_exit


def test_stage_arguments():
    from distributed_neural_networks_amd.config import StopConfig
    model, n, sd, V = _tiny()
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    mid = TorchStage(model, sd, 0, n - 2, True, False,
                     sampling=(0.0, 0, 0, 1.0, 0.0, 1.0, 0.0, 0.0, 0, StopConfig((1,), (), 0, 1)))
    assert mid.stop is None and mid.stop_state is None  # only a last stage acts on the keys
    off = _stage(model, sd, n, None)
    assert off.stop is None and off.stop_state is None
    with pytest.raises(ValueError, match="no stop conditions"):
        off.stop_begin(0, 2)
    on = _stage(model, sd, n, StopConfig((1,), (), 0, 1))
    with pytest.raises(ValueError, match="no stop_begin"):
        on.step(torch.zeros((1, 3), dtype=torch.int64), 0, 1, 3)


# ---------------------------------------------------------------------- two gloo ranks vs one process
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run_nodes(cfg, n, extra0=(), timeout=120, env=ENV):
    procs = []
    for i in range(1, n):
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", f"node{i + 1}",
                                       "--config", str(cfg), "--serve_seconds", "90"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    try:
        r0 = subprocess.run([sys.executable, os.path.join(ROOT, "node.py"), "--node_id", "node1", "--config", str(cfg),
                             "--input_image", "none.png", "--shutdown_pipeline", *extra0], env=env,
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
    """The padded tokens arrive on rank 0 over the back-edge; the last rank
    prints the FINISH line; both equal what one process with both stages gives."""
    from distributed_neural_networks_amd import checkpoint as ckpt
    from distributed_neural_networks_amd.config import parse_pipeline
    from distributed_neural_networks_amd.models import default_ranges
    from distributed_neural_networks_amd.runtime.scheduler import DecodeRing, RingLinks
    from distributed_neural_networks_amd.runtime.stages import TorchStage
    from distributed_neural_networks_amd.runtime.generate import make_prompts
    model, steps = "gpt2-tiny", 10
    ranges = default_ranges(model, 2)
    c = {"nodes": [{"id": f"node{i + 1}", "address": f"127.0.0.1:{_free_port()}", "part_index": i} for i in range(2)],
         "model_weights": "synthetic:1", "num_parts": 2, "return_to_node_id": "node1", "transport": "gloo",
         "model": model, "seq_len": 12, "decode_steps": steps, "micro_batch_size": 2, "num_microbatches": 2,
         "temperature": 0.8, "top_k": 20, "top_p": 0.9, "seed": 7}
    prompt = make_prompts(parse_pipeline(c), None)  # the CLI's own seeded prompts: four different rows

    def one_process(stop):
        samp = (0.8, 20, 7, 0.9, 0.0, 1.0, 0.0, 0.0, 0, stop)
        stages = [TorchStage(model, ckpt.random_stage_state_dict(model, a, b, i == 0, i == 1, 1), a, b, i == 0,
                             i == 1, sampling=samp) for i, (a, b) in enumerate(ranges)]
        ring = DecodeRing(stages, RingLinks(), 1, 2, 2, use_graphs=False, early_exit=False)
        return ring.generate([prompt[:2], prompt[2:]], prompt.shape[1], steps), ring

    free, _ = one_process(None)
    ids, seqs, lens, why = choose_stops(free)  # a row stops midway on the id, one on the sequence, one never
    c.update({"eos_token_id": ids[0], "stop_sequences": [list(seqs[0])], "pad_token_id": 3})
    stop = parse_pipeline(c).stop
    want_t, ring = one_process(stop)
    want = ring.finished()
    exp_t, exp_len, exp_why = expected_from(free, stop)
    assert torch.equal(want_t, exp_t) and torch.equal(want["length"], exp_len) and want["reason"] == exp_why
    assert want["reason"] == why and any(w == ("token", 0) for w in why) and any(w == ("sequence", 0) for w in why) \
        and any(w is None for w in why)
    cfg = tmp_path / "cfg.json"
    cfg.write_text(json.dumps(c))
    r0, outs = _run_nodes(cfg, 2)
    assert r0.returncode == 0, r0.stdout[-3000:] + r0.stderr[-2000:] + "".join(o[-2000:] for o in outs)
    toks = torch.tensor(json.loads(r0.stdout.split("generated tokens:")[1].strip().splitlines()[0]), dtype=torch.int32)
    assert torch.equal(toks, want_t)
    assert "FINISH" not in r0.stdout  # rank 0 has the tokens, the last rank the finish record
    line = json.loads(outs[0].split("FINISH ")[1].splitlines()[0])
    assert line["length"] == want["length"].tolist() and line["pad_token_id"] == 3
    assert [None if r is None else tuple(r) for r in line["reason"]] == want["reason"]
    metrics = json.loads(r0.stdout.split("METRICS ")[1].splitlines()[0])
    assert metrics["decode_steps"] == steps - 1  # rings of several groups run all their rounds
