"""TEST INFRASTRUCTURE: the library's frame queue (x264_vs2008_amd.lookahead.Lookahead over csrc/lookahead_host.hip) driven with made-up
costs, and everything it answers written down -- tests/test_lookahead_queue_trace.py holds the library to the trace recorded in
tests/golden/look_queue_trace.npz.  No pictures, no oracle, no reference: a cost is a pure function of (seed, b, p0, p1), an integer
hash scaled to the magnitudes real clips give, so that the slice-type decisions (b-adapt 0 / 1 / 2, the keyint limit, the scene cuts),
the rate control (CQP, CRF) and the order of the questions the decisions ask are all exercised and all reproducible.

What one run does beyond put / get / set_cost / end, at seeded points:
  * instead of end() on a P picture, scenecut() (the post-encode scene cut's "give up"), in configurations without the pre-encode cut;
  * save(), then either (ahead=True) end() and several put / get / end calls followed by restore(), or (ahead=False) the same number
    of put calls alone.  Both leave the queue in the same state if restore() is right, so both runs must give the same trace.

`PYTHONPATH=. python tests/look_trace.py` rewrites the fixture from the library as built; with the argument `check` it only prints what the
fixture covers."""
import os
import struct
import sys

import numpy as np

from paths import GOLDEN
from x264_vs2008_amd import lookahead as LA

FIXTURE = os.path.join(GOLDEN, "look_queue_trace.npz")
SEEDS = list(range(200))
SCENECUT, AHEAD = 4, 5                      # records of the trace beside get()'s kinds (LA.NONE / FRAME / NEED / END)
FRAME_FIELDS = [name for name, _ in LA.Frame._fields_]
BFRAMES_ADAPT2 = (1, 2, 3, 5, 8, 16)
SIZES = ((20, 15), (8, 6), (45, 36))
ROOM = 65                                   # pictures one decision looks at, at the most (X264_BFRAME_MAX * 4 + 1): never more are put and not yet coded


def mix(*words):
    """A 32-bit integer hash of a few integers."""
    h = 0x9E3779B9
    for w in words:
        h = ((h ^ (w & 0xFFFFFFFF)) * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
    return h


def config(seed):
    g = seed % 8                            # 0-5: b-adapt 2 with each B count; 6: b-adapt 1; 7: fixed B pattern
    if g < 6:
        b_adapt, bframes = 2, BFRAMES_ADAPT2[g]
    elif g == 6:
        b_adapt, bframes = 1, 1 + mix(seed, 1) % 4
    else:
        b_adapt, bframes = 0, mix(seed, 1) % 4
    h = mix(seed, 2)
    pre = h & 1
    mb_w, mb_h = SIZES[(h >> 1) % 3]
    frames = 40 + (h >> 3) % 81
    if bframes == 16:                       # a delay of 64 pictures: keep some decisions that are not the flush's
        frames = 80 + (h >> 3) % 41
    elif bframes >= 5:                      # (the long searches ask the most questions: shorter streams keep the fixture's size down)
        frames = 40 + (h >> 3) % 41
    return dict(seed=seed, b_adapt=b_adapt, bframes=bframes, pre_scenecut=pre, scenecut_threshold=40, mb_w=mb_w, mb_h=mb_h, frames=frames,
                keyint=(250, 250, 12, 7, 30)[(h >> 10) % 5], keyint_min=(0, 0, 2)[(h >> 13) % 3], crf=(None, 18.0, None, 27.5)[(h >> 15) % 4],
                qp=20 + (h >> 17) % 16, bframe_bias=(0, 0, 20, -30)[(h >> 21) % 4], answer_speculative=(h >> 23) & 1,
                cuts=sorted({5 + mix(seed, 3, i) % (frames - 5) for i in range((h >> 24) % 4)}))


def params(c):
    return LA.make_params(c["mb_w"], c["mb_h"], bframes=c["bframes"], b_adapt=c["b_adapt"], bframe_bias=c["bframe_bias"], keyint_max=c["keyint"],
                          keyint_min=c["keyint_min"], scenecut_threshold=c["scenecut_threshold"], pre_scenecut=c["pre_scenecut"], crf=c["crf"],
                          qp=c["qp"], qp_min=0)


def cost(c, b, p0, p1):
    """(score, intra_mbs, cost00) of x264_slicetype_frame_cost(p0, p1, b): an intra cost per picture, inter costs that grow with the
    distance to the nearer reference and with the activity of the 24-picture segment, a B picture cheaper than a P by the segment's factor,
    and a reference on the far side of a scene change useless.  Integers only."""
    seed = c["seed"]
    nmb = (c["mb_w"] - 2) * (c["mb_h"] - 2)
    intra = nmb * (300 + mix(seed, 4, b) % 300)
    if b == p0 and b == p1:
        return intra, 0, intra
    u = mix(seed, 5, b, p0, p1)
    seg = mix(seed, 6, b // 24)
    activity = (30, 80, 160, 300, 500, 900)[seg % 6]                 # of 1024: the share of the intra cost one picture of distance costs
    cut0 = any(p0 < t <= b for t in c["cuts"])                       # a scene change between the past reference and the picture
    cut1 = any(b < t <= p1 for t in c["cuts"])
    if b == p1:
        dist, share = (None if cut0 else b - p0), 256
    else:
        near = [d for d, cut in ((b - p0, cut0), (p1 - b, cut1)) if not cut]
        dist, share = (min(near) if near else None), (60, 100, 150, 210)[(seg >> 8) % 4]
    if dist is None:
        frac = 960 + u % 256                                         # no better than intra
    else:
        frac = min(1100, activity * 2 * dist // (dist + 2) * share // 256 * (192 + u % 128) // 256)
    score = intra * frac // 1024
    r = min(1024, frac)
    return score, (nmb * r * r) >> 20 if b == p1 else 0, intra


def float_bits(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def pump(la, c, flushing, trace):
    """get() until it stops asking, every need answered (the speculative ones in half the configurations); every get is written down."""
    while True:
        kind, fr, needs = la.get(flushing)
        if trace is not None:
            if kind == LA.NEED:
                trace.append((kind,) + tuple(x for nd in needs for x in nd))
            elif kind == LA.FRAME:
                trace.append((kind,) + tuple(float_bits(fr.f_qpm) if k == "f_qpm" else getattr(fr, k) for k in FRAME_FIELDS))
            else:
                trace.append((kind,))
        if kind != LA.NEED:
            return kind, fr
        assert needs and needs[0][5] == 0
        for (b, p0, p1, ds0, ds1, spec) in needs:
            if not spec or c["answer_speculative"]:
                la.set_cost(b, p0, p1, *cost(c, b, p0, p1), speculative=spec)


def run(lib, seed, ahead):
    """The trace of one configuration: a list of tuples -- (kind,), (NEED, b, p0, p1, do_search0, do_search1, speculative, ...),
    (FRAME, every field of x264hip_look_frame with f_qpm as its bits), (SCENECUT, what scenecut() returned), (AHEAD, pictures put between
    save() and restore(), or -1 where the state did not fit)."""
    c = config(seed)
    la = LA.Lookahead(lib, params(c))
    trace, fed, coded, step, n = [], 0, 0, 0, c["frames"]
    while True:
        flushing, step = fed >= n, step + 1
        if not flushing and mix(seed, 8, step) % 6:           # (now and then no picture arrives: the queue runs below its delay)
            la.put()
            fed += 1
        kind, fr = pump(la, c, flushing, trace)
        if kind == LA.NONE or (kind == LA.END and not flushing):     # (END before the flush: the queue has run empty, pictures are still to come)
            continue
        if kind == LA.END:
            break
        point = mix(seed, 7, coded)
        if point % 7 == 0:                                           # the run-ahead beside the sweep of the picture in flight, and back
            state, k = la.save(), min(1 + (point >> 8) % 6, n - fed, ROOM - (fed - coded))
            trace.append((AHEAD, k if state is not None else -1))
            if state is not None and ahead:
                la.end()
                for i in range(k):
                    la.put()
                    if pump(la, c, False, None)[0] == LA.FRAME and (i < k - 1 or (point >> 12) & 1):
                        la.end()
                la.restore(state)
            elif state is not None:
                for i in range(k):
                    la.put()
            if state is not None:
                fed += k
        if not c["pre_scenecut"] and fr.type == LA.TYPE_P and (point >> 16) % 5 == 0:
            trace.append((SCENECUT, la.scenecut()))
            kind, fr = pump(la, c, flushing, trace)
            assert kind == LA.FRAME
        la.end()
        coded += 1
    la.close()
    return trace


# ---- the fixture: every trace as integer arrays -------------------------------------------------------------------------------------------
def encode(traces):
    """{seed: trace} -> arrays: one kind per record, the needs / frames / events in tables of their own, narrow types, a field per row.  A need
    is (b as its difference to the need before, modulo 256; b - p0; p1 - b; do_search and speculative as bits 0, 1, 2): what compresses."""
    kinds, n_need, need, frame, event, start = [], [], [], [], [], [0]
    for seed in sorted(traces):
        for rec in traces[seed]:
            kinds.append(rec[0])
            if rec[0] == LA.NEED:
                n_need.append((len(rec) - 1) // 6)
                need += [(b, b - p0, p1 - b, ds0 | ds1 << 1 | spec << 2) for b, p0, p1, ds0, ds1, spec in zip(*[iter(rec[1:])] * 6)]
            elif rec[0] == LA.FRAME:
                frame.append(rec[1:])
            elif rec[0] in (SCENECUT, AHEAD):
                event.append(rec[1])
        start.append(len(kinds))
    need = np.array(need, np.int64).reshape(-1, 4).T
    need[0] = np.diff(need[0], prepend=0)
    need = np.ascontiguousarray(need.astype(np.uint8))
    return dict(seeds=np.array(sorted(traces), np.int32), start=np.array(start, np.int32), kind=np.array(kinds, np.uint8),
                n_need=np.array(n_need, np.uint8), need=need,
                frame=np.ascontiguousarray(np.array(frame, np.int32).reshape(-1, len(FRAME_FIELDS)).T), event=np.array(event, np.int16))


def decode(g):
    """encode()'s arrays -> {seed: trace}"""
    need = g["need"].astype(np.int64)
    need[0] = np.cumsum(need[0]) % 256
    kinds, n_need, need, frame, event = g["kind"].tolist(), g["n_need"].tolist(), need.T.tolist(), g["frame"].T.tolist(), g["event"].tolist()
    i_nn = i_need = i_frame = i_event = 0
    traces = {}
    for seed, lo, hi in zip(g["seeds"].tolist(), g["start"][:-1].tolist(), g["start"][1:].tolist()):
        tr = []
        for kind in kinds[lo:hi]:
            if kind == LA.NEED:
                rec = [kind]
                for b, d0, d1, bits in need[i_need:i_need + n_need[i_nn]]:
                    rec += [b, b - d0, b + d1, bits & 1, bits >> 1 & 1, bits >> 2]
                i_need += n_need[i_nn]
                i_nn += 1
                tr.append(tuple(rec))
            elif kind == LA.FRAME:
                tr.append((kind,) + tuple(frame[i_frame]))
                i_frame += 1
            elif kind in (SCENECUT, AHEAD):
                tr.append((kind, event[i_event]))
                i_event += 1
            else:
                tr.append((kind,))
        traces[seed] = tr
    return traces


def coverage(traces):
    """What the traces reach, for the test's conditions:
      b_runs: in the b-adapt 2 configurations, the lengths of the runs of B pictures handed out after a picture that is none;
      cut_short: path pricings the threshold ended early.  Pricing a path asks a P picture's cost (p0, p1, p1) and then, in the same pass,
          the costs (p0, p1, b) of every B picture between them, unless the running cost passed the threshold; nothing else in a b-adapt 2
          decision under constant QP asks for a cost over a span longer than 1.  So a span whose P cost was asked while one of its B costs
          never was, in the whole run, is a pricing that asked fewer questions than its path has;
      restores_with_puts / scenecuts: the save / restore legs with pictures put in between, and what scenecut() returned."""
    b_runs, cut_short, restores, scenecuts = set(), 0, 0, set()
    for seed, tr in traces.items():
        c = config(seed)
        asked, run_len = set(), None
        for rec in tr:
            if rec[0] == LA.NEED:
                asked |= {(b, p0, p1) for b, p0, p1 in zip(rec[1::6], rec[2::6], rec[3::6])}
            elif rec[0] == LA.FRAME and c["b_adapt"] == 2:
                if rec[1 + FRAME_FIELDS.index("type")] == LA.TYPE_B:
                    run_len += 1
                else:
                    b_runs |= {run_len} - {None}
                    run_len = 0
            elif rec[0] == SCENECUT:
                scenecuts.add(rec[1])
            elif rec[0] == AHEAD and rec[1] > 0:
                restores += 1
        b_runs |= {run_len} - {None}
        if c["b_adapt"] == 2 and c["crf"] is None:
            cut_short += sum(1 for (b, p0, p1) in asked if b == p1 and any((m, p0, p1) not in asked for m in range(p0 + 1, p1)))
    return dict(b_runs=sorted(b_runs), cut_short=cut_short, restores_with_puts=restores, scenecuts=sorted(scenecuts))


def main():
    from x264_vs2008_amd import lib as L
    if sys.argv[1:] == ["check"]:
        with np.load(FIXTURE) as g:
            traces = decode(g)
    else:
        lib = L.open_library()
        traces = {seed: run(lib, seed, True) for seed in SEEDS}
        assert all(run(lib, seed, False) == traces[seed] for seed in SEEDS), "a run that never ran ahead gives another trace"
        arrays = encode(traces)
        assert decode(arrays) == traces
        np.savez_compressed(FIXTURE, **arrays)
    print("%s: %d bytes, %d configurations, %d records, %s" % (FIXTURE, os.path.getsize(FIXTURE), len(traces), sum(len(t) for t in traces.values()),
                                                             coverage(traces)))


if __name__ == "__main__":
    main()
