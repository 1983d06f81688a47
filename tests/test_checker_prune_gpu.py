"""The QueueChecker's prune of the packed intent queue (check_stream_kernel, q = 0): the
packed items stay in LDS, the select works on keys derived from them (the transmit count
from pass 1's counts, then 10-bit digits of the folded length / age bits over that count's
items), and pass 2 writes the kept items back in index order, each wave a contiguous run of
the tail.  Every case is bit-exact against the oracle world, compared after the tick and after
every one of the rounds that follow it, so the deferred path's recent mode runs on the seals
the prune leaves.

Shape: 300 members, 48 subjects, every member originating an intent each round and 1000 bytes
of gossip per target, so a member's intent queue grows by ~29 items a round (the oracle on
the CPU: 855 items after 30 rounds, 1 740 after 60, min / max within +-10 %)."""
import ctypes as C

import numpy as np
import pytest

import gossip_harness as H
import oracle_ffi as O
from ruserf_amd import gossip as G
from ruserf_amd import workload as W

pytestmark = pytest.mark.gpu
L = O.lib()

N, S, QCAP = 300, 48, 64
# pass 2: four waves, each a contiguous quarter of the tail in steps of 4 x 64 items -- tails up
# to 1024 items take one step per wave, longer ones more
PASS2_BATCH = 1024


def grown(rounds, seed):
    """(engine, oracle world, workload) after `rounds` rounds without a tick"""
    cfg = G.GossipConfig(n_members=N, n_subjects=S, queue_cap=QCAP, queue_depth=(8192, 0, 0), gossip_limit=1000,
                         gossip_overhead=2, max_rumors=1 << 16, event_buffer_size=64, query_buffer_size=64, slot_k=1)
    total = rounds + 64  # (room for the rounds after the ticks)
    subj, acts, ml = W.intents_workload(N, S, total, rate=1.0, seed=seed)
    g = G.GossipEngine(cfg)
    g.set_subjects(subj)
    g.init_views(*W.initial_views(S))
    w = H.oracle_world(cfg, subj, W.initial_views(S))
    run(g, w, (acts, ml), 0, rounds, compare=False)
    return g, w, (acts, ml)


def same(g, w, ctx):
    e, o = H.deep_states(g, w)
    H.assert_same(e, o, ctx)


def run(g, w, wl, t0, t1, compare=True):
    acts, ml = wl
    for t in range(t0, t1):
        g.round(t, ml[t], acts[t])
        H.oracle_round(w, t, ml[t], acts[t], threads=16)
        if compare:
            same(g, w, f"round {t}")


def tick(g, w, mx, mn, ctx):
    """one QueueChecker tick over every member on both sides: the counts and the state"""
    got = g.check_queues(mx, mn, 128)
    exp = (C.c_uint64 * 9)()
    L.orc_check_queues(C.byref(w), mx, mn, 128, exp)
    assert list(got["queued"]) + list(got["warn"]) + list(got["pruned"]) == list(exp), (ctx, mx, mn)
    same(g, w, f"{ctx}: tick to {mx}")
    return int(got["pruned"][0])


def intent_items(w):
    """the oracle's intent queues: (live mask, transmits, length, seq), each [N, width]"""
    q = w.qcap
    f = lambda p, t: O.arr(p, N * 3 * q, t).reshape(N, 3, q)[:, 0, :H.world_width(w)]  # noqa: E731
    return f(w.q_rumor, np.uint32) != 0xFFFFFFFF, f(w.q_tx, np.uint16), f(w.q_len, np.uint16), f(w.q_seq, np.uint32)


def close(g, w):
    g.close()
    L.orc_world_free(C.byref(w))


def test_multi_digit_select_two_periods_bit_exact():
    """Queues of 1.6-1.9k items pruned to 1 100, grown for another period to ~2.2k and pruned
    again.  At both ticks every ticked queue's keys differ in the transmit count, in the length
    and in more than one byte of seq (asserted on the oracle's queues), so the select takes the
    transmit-count step and more than one digit of the folded length / age bits."""
    mx, period = 1100, 40
    g, w, wl = grown(60, seed=79)
    t = 60
    for k in range(2):
        live, tx, ln, sq = intent_items(w)
        lens = g.queue_lengths()[:, 0]
        assert np.array_equal(lens, live.sum(1))
        assert lens.min() > mx and 1500 <= np.median(lens) <= 2500, (lens.min(), np.median(lens))
        for l in range(N):
            m = live[l]
            assert len(np.unique(tx[l][m])) > 1 and len(np.unique(ln[l][m])) > 1, l
            diff = np.bitwise_or.reduce(sq[l][m] ^ sq[l][m][0])
            assert sum(1 for b in range(4) if (int(diff) >> (8 * b)) & 0xFF) > 1, (l, hex(int(diff)))
        assert tick(g, w, mx, 0, f"tick {k}") > 0
        assert int(g.queue_lengths()[:, 0].max()) == mx
        if k == 0:
            run(g, w, wl, t, t + 3)
            run(g, w, wl, t + 3, t + period, compare=False)
            t += period
        else:
            run(g, w, wl, t, t + 3)
    close(g, w)


def test_pass2_batch_boundary_bit_exact():
    """Ticked tails on both sides of one pass-2 step per wave (1 024 tail items), and lengths
    that are no multiple of 64: the last step of a wave's run is partial, and the last waves'
    runs are shorter than the first's."""
    g, w, wl = grown(37, seed=80)
    lens = g.queue_lengths()[:, 0]
    tails, _ = g.tails(0)
    # (a queue is its 64-slot head plus its tail: below the batch for sure, above it for sure)
    assert (lens <= PASS2_BATCH).any() and (lens > PASS2_BATCH + QCAP).any(), (lens.min(), lens.max())
    assert (tails < PASS2_BATCH).any() and (tails > PASS2_BATCH).any() and (tails % 64 != 0).any()
    assert (lens % 64 != 0).any()
    assert tick(g, w, 600, 0, "batch") > 0
    run(g, w, wl, 37, 40)
    close(g, w)


def test_keep_below_queue_cap_bit_exact():
    """max 40 against the 64-slot head: the 40th key lies inside the head, the head's suffix is
    cleared and the tail empties (at nearly every member); then several rounds on the part-full
    heads."""
    g, w, wl = grown(12, seed=81)
    assert int(g.queue_lengths()[:, 0].min()) > QCAP
    assert tick(g, w, 40, 0, "below the head") > 0
    assert int(g.queue_lengths()[:, 0].max()) == 40
    # (a head need not hold its queue's smallest keys -- items spilled from it may precede its
    # last ones -- so a few tails keep some items; nearly all empty, their seals with them)
    tails, sealed = g.tails(0)
    assert int((tails == 0).sum()) > N * 9 // 10 and int(tails.max()) < 40, np.flatnonzero(tails)
    assert int(sealed[tails == 0].max()) == 0
    run(g, w, wl, 12, 17)
    close(g, w)


def test_one_item_over_bit_exact():
    """max chosen from the observed lengths so that some member holds exactly max + 1 items (one
    item goes) and another exactly max (not listed: its queue is left as it is)."""
    g, w, wl = grown(20, seed=82)
    lens = g.queue_lengths()[:, 0].astype(np.int64)
    have = set(lens.tolist())
    cand = sorted(m for m in have if m + 1 in have)
    assert cand, sorted(have)
    mx = cand[len(cand) // 2]
    at, over = int(np.flatnonzero(lens == mx)[0]), int(np.flatnonzero(lens == mx + 1)[0])
    tails0, sealed0 = g.tails(0)
    before = g.queues_rows(at, 1, mx + 1)
    assert tick(g, w, mx, 0, "one over") > 0
    after = g.queues_rows(at, 1, mx + 1)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)  # the member at its max: untouched
    tails1, sealed1 = g.tails(0)
    assert tails1[at] == tails0[at] and sealed1[at] == sealed0[at]
    lens1 = g.queue_lengths()[:, 0]
    assert lens1[over] == mx and lens1[at] == mx
    run(g, w, wl, 20, 23)
    close(g, w)


def test_per_member_max_packed_queue_bit_exact():
    """min_queue_depth > 0: each member's own max, max(2 x the members it knows, min), on the
    packed queue (the views differ per member through the prunes, so the maxes do)."""
    g, w, wl = grown(30, seed=83)
    lens0 = g.queue_lengths()[:, 0]
    mn = 530  # (the oracle on the CPU: 2 x known spans 512..548, 175 members at or below 530)
    assert tick(g, w, 4096, mn, "per member") > 0
    lens1 = g.queue_lengths()[:, 0]
    assert (lens1 < lens0).all() and len(np.unique(lens1)) > 1 and int(lens1.min()) == mn, np.unique(lens1)
    run(g, w, wl, 30, 33)
    close(g, w)
