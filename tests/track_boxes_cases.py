"""The cases of the box-linking tests and a restatement of the definition at the head of csrc/track_boxes.h in plain Python:
the SEQUENTIAL greedy matching, with every intersection over union an exact `fractions.Fraction`, one pair taken at a time.  The
library never works this way (it matches in rounds of mutual best choices, on products of int64), so agreement is not by shared
code.  `wrong` selects another rule: four wrong ones, each of which a named case tells from the right one, and `det_first` (a tie to the
smaller detection index before the smaller track id), which is a different order of the pairs but provably the same matching.  Importable without a GPU and
without the library."""
from fractions import Fraction

import numpy as np

CANARY = -0x35014542
LIVE_MAX, MAX_COORD, HDR, REC = 128, 16384, 8, 13
STATE_WORDS = HDR + LIVE_MAX * REC
BAD_BOX, TRACKS_FULL, LIVE_FULL, ORDER, BAD_STATE = 1, 2, 4, 8, 16
DEFAULTS = dict(iou=(3, 10), max_gap=2, predict=1, max_tracks=16)
WRONG = ("floor", "tie_last", "gt", "first_fit", "det_first")


def tdiv(a, b):
    """C++'s integer division: towards zero (Python's // floors)."""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


class Video:
    """What the restatement knows of a video between calls."""

    def __init__(self):
        self.next_id, self.flags, self.next_t, self.linked = 0, 0, 0, 0
        self.live = []                                             # dicts id, first, last, hits, prev, box, pbox - ascending id
        self.rows = {}                                             # id -> (first_t, last_t, hits) of every track so far

    def state(self):
        s = np.zeros((STATE_WORDS,), dtype=np.int32)
        s[:5] = [self.next_id, len(self.live), self.flags, self.next_t, self.linked]
        for a, r in enumerate(self.live):
            s[HDR + a * REC:HDR + (a + 1) * REC] = [r["id"], r["first"], r["last"], r["hits"], r["prev"], *r["box"], *r["pbox"]]
        return s

    def tracks(self, N):
        out = np.zeros((N, 4), dtype=np.int32)
        for i, row in self.rows.items():
            out[i, :3] = row
        return out

    def stats(self, extra=0):
        return np.asarray([self.next_id, len(self.live), self.linked, self.flags | extra], dtype=np.int32)


def _area(b):
    return (b[2] - b[0]) * (b[3] - b[1])


def _inter(a, b):
    w, h = min(a[2], b[2]) - max(a[0], b[0]), min(a[3], b[3]) - max(a[1], b[1])
    return w * h if w > 0 and h > 0 else 0


def _expected(r, t, predict, wrong):
    if not predict or r["hits"] < 2:
        return r["box"]
    div = (lambda a, b: a // b) if wrong == "floor" else tdiv
    (x0, y0, x1, y1), p = r["box"], r["pbox"]
    dx = div(((x0 + x1) - (p[0] + p[2])) * (t - r["last"]), 2 * (r["last"] - r["prev"]))
    dy = div(((y0 + y1) - (p[1] + p[3])) * (t - r["last"]), 2 * (r["last"] - r["prev"]))
    return (x0 + dx, y0 + dy, x1 + dx, y1 + dy)


def link(video, boxes, stats, t0=0, iou=(3, 10), max_gap=2, predict=1, max_tracks=16, wrong=None):
    """One call on one video: boxes int [T, K, 4], stats int [T, 4] -> (ids int32 [T, K], out_stats int32 [4]); `video` moves on."""
    boxes, stats = np.asarray(boxes).astype(np.int64), np.asarray(stats)
    T, K = boxes.shape[:2]
    ids = np.full((T, K), -1, dtype=np.int32)
    if T > 0 and t0 < video.next_t:
        return ids, video.stats(ORDER)
    thr = Fraction(*iou)
    for j in range(T):
        t = t0 + j
        n = min(max(int(stats[j, 0]), 0), K)
        for r in video.live:
            video.rows[r["id"]] = (r["first"], r["last"], r["hits"])
        video.live = [r for r in video.live if t - r["last"] <= max_gap + 1]
        dets = [tuple(int(v) for v in boxes[j, d]) for d in range(n)]
        ok = [min(b) >= 0 and max(b) <= MAX_COORD and b[2] > b[0] and b[3] > b[1] for b in dets]
        if not all(ok):
            video.flags |= BAD_BOX
        exp = [_expected(r, t, predict, wrong) for r in video.live]
        free_a, free_d = list(range(len(video.live))), [d for d in range(n) if ok[d]]
        match = {}

        def iou_of(a, d):
            i = _inter(exp[a], dets[d])
            return Fraction(i, _area(exp[a]) + _area(dets[d]) - i)

        def eligible(a, d):
            v = iou_of(a, d)
            return v > 0 and (v > thr if wrong == "gt" else v >= thr)
        if wrong == "first_fit":                                   # tracks in id order, each its best detection
            for a in list(free_a):
                c = [d for d in free_d if eligible(a, d)]
                if c:
                    d = max(c, key=lambda d: (iou_of(a, d), -d))
                    match[d] = a
                    free_d.remove(d)
        else:
            while True:
                c = [(a, d) for a in free_a for d in free_d if eligible(a, d)]
                if not c:
                    break
                tie = {"det_first": lambda p: (iou_of(*p), -p[1], -p[0]), "tie_last": lambda p: (iou_of(*p), p[0], -p[1])}.get(
                    wrong, lambda p: (iou_of(*p), -p[0], -p[1]))
                a, d = max(c, key=tie)                             # the ids of the live tracks rise with their position
                match[d] = a
                free_a.remove(a)
                free_d.remove(d)
        n_live = len(video.live)
        for d in range(n):
            if not ok[d]:
                continue
            if d in match:
                r = video.live[match[d]]
                r.update(pbox=r["box"], prev=r["last"], box=dets[d], last=t, hits=r["hits"] + 1)
                ids[j, d] = r["id"]
                video.linked += 1
            elif video.next_id == max_tracks:
                video.flags |= TRACKS_FULL
            elif n_live == LIVE_MAX:
                video.flags |= LIVE_FULL
            else:
                video.live.append(dict(id=video.next_id, first=t, last=t, hits=1, prev=t, box=dets[d], pbox=dets[d]))
                ids[j, d] = video.next_id
                video.next_id += 1
                n_live += 1
        video.next_t = t + 1
    for r in video.live:
        video.rows[r["id"]] = (r["first"], r["last"], r["hits"])
    return ids, video.stats()


def tables(frames, K, n=None):
    """Lists of boxes per frame -> (boxes int32 [T, K, 4] zero-padded, stats int32 [T, 4]) as ops.foreground_boxes writes them; n
    replaces the counts."""
    T = len(frames)
    boxes, stats = np.zeros((T, K, 4), dtype=np.int32), np.zeros((T, 4), dtype=np.int32)
    for f, fr in enumerate(frames):
        for k, b in enumerate(fr):
            boxes[f, k] = b
        stats[f, 0] = len(fr) if n is None else n[f]
        stats[f, 1] = stats[f, 0]
    return boxes, stats


def run(case, wrong=None):
    """The restatement on a named case, one call from a fresh video -> (ids, tracks, out_stats, state)."""
    p = dict(DEFAULTS, **case.get("params", {}))
    v = Video()
    boxes, stats = tables(case["frames"], case["K"], case.get("n"))
    ids, out = link(v, boxes, stats, case.get("t0", 0), wrong=wrong, **p)
    return ids, v.tracks(p["max_tracks"]), out, v.state()


def want_ids(case):
    """The ids written beside the case as the [T, K] table."""
    T, K = len(case["frames"]), case["K"]
    out = np.full((T, K), -1, dtype=np.int32)
    for f, row in enumerate(case["want"]):
        out[f, :len(row)] = row
    return out


def _sq(x, y, w=10, h=10):
    return (x, y, x + w, y + h)


def _crossing():
    frames, want = [], []
    for f in range(9):
        a, b = _sq(10 * f, 0, 20, 20), _sq(80 - 10 * f, 10, 20, 20)   # A goes right, B goes left, they share pixels in the middle
        frames.append([a, b] if f < 5 else [b, a])
        want.append([0, 1] if f < 5 else [1, 0])
    return frames, want


_ROW0, _ROW1 = [_sq(20 * k, 0) for k in range(64)], [_sq(20 * k, 40) for k in range(64)]

CASES = [
    dict(name="crossing", K=4, frames=_crossing()[0], want=_crossing()[1], flags=0),
    # one detection half way between two tracks: both pairs 50 / 150 - the smaller track id takes it, track 1 goes unseen
    dict(name="tie_by_track_id", K=4, frames=[[_sq(0, 0), _sq(10, 0)], [_sq(5, 0)]], want=[[0, 1], [0]], flags=0),
    # two detections at 50 / 150 from one track: the smaller detection index takes it, the other founds a track
    dict(name="tie_by_detection_index", K=4, frames=[[_sq(10, 0)], [_sq(15, 0), _sq(5, 0)]], want=[[0], [0, 1]], flags=0),
    dict(name="threshold_exactly_met", K=2, params=dict(iou=(1, 3)), frames=[[(0, 0, 100, 1)], [(50, 0, 150, 1)]], want=[[0], [0]], flags=0),
    dict(name="threshold_missed_by_one", K=2, params=dict(iou=(1, 3)), frames=[[(0, 0, 100, 1)], [(50, 0, 151, 1)]], want=[[0], [1]], flags=0),
    dict(name="gap_of_max_gap_bridged", K=2, frames=[[_sq(0, 0)], [], [], [_sq(0, 0)]], want=[[0], [], [], [0]], flags=0),
    dict(name="gap_of_max_gap_plus_1_not_bridged", K=2, frames=[[_sq(0, 0)], [], [], [], [_sq(0, 0)]], want=[[0], [], [], [], [1]], flags=0),
    # 20 wide at 8 a frame, unseen for two frames: the last box (8..28) misses (32..52), the predicted one is it
    dict(name="predict_bridges", K=2, frames=[[_sq(0, 0, 20)], [_sq(8, 0, 20)], [], [], [_sq(32, 0, 20)]], want=[[0], [0], [], [], [0]], flags=0),
    dict(name="no_predict_misses", K=2, params=dict(predict=0), frames=[[_sq(0, 0, 20)], [_sq(8, 0, 20)], [], [], [_sq(32, 0, 20)]],
         want=[[0], [0], [], [], [1]], flags=0),
    # (x0 + x1) goes 30 -> 27: tdiv(-3, 2) = -1 puts the expected box at 8..17, 60 / 120 with 11..20: met; floor's -2 gives 50 / 130
    dict(name="negative_velocity_truncates", K=2, params=dict(iou=(1, 2)), frames=[[(10, 0, 20, 10)], [(9, 0, 18, 10)], [(11, 0, 20, 10)]],
         want=[[0], [0], [0]], flags=0),
    dict(name="birth_and_match_in_one_frame", K=4, frames=[[_sq(50, 50)], [_sq(0, 0), _sq(52, 50)]], want=[[0], [1, 0]], flags=0),
    dict(name="empty_frames", K=2, frames=[[], [], [_sq(3, 3)], []], want=[[], [], [0], []], flags=0),
    dict(name="count_above_K_is_clamped", K=2, frames=[[_sq(0, 0), _sq(30, 0)], [_sq(1, 0), _sq(31, 0)], [_sq(2, 0)]], n=[5, 1 << 30, -3],
         want=[[0, 1], [0, 1], []], flags=0),
    # 64 + 64 tracks, 64 detections against all 128 of them twice, then one more box with 128 live
    dict(name="live_full", K=64, params=dict(max_tracks=256), frames=[_ROW0, _ROW1, _ROW1, _ROW0, [_sq(0, 100)] + _ROW1[:5]],
         want=[list(range(64)), list(range(64, 128)), list(range(64, 128)), list(range(64)), [-1] + list(range(64, 69))], flags=LIVE_FULL),
    dict(name="tracks_full", K=4, params=dict(max_tracks=2), frames=[[_sq(0, 0), _sq(30, 0), _sq(60, 0)], [_sq(60, 0), _sq(30, 0)]],
         want=[[0, 1, -1], [-1, 1]], flags=TRACKS_FULL),
    # empty, negative, beyond 16384; the largest box there is takes part (the products' bound)
    dict(name="bad_box", K=4, frames=[[(5, 5, 5, 10), (-1, 0, 10, 10), (0, 0, 16385, 10), (0, 0, 16384, 16384)],
                                      [(1, 1, 16384, 16384), (3, 4, 2, 9)]], want=[[-1, -1, -1, 0], [0, -1]], flags=BAD_BOX),
    # best first against track order: track 0 shares pixels with both detections and likes d1 better (100 / 300 against 80 / 320),
    # but d1 and track 1 are the better pair (180 / 220): track 0 is left with d0.  In track order d1 would go to track 0
    dict(name="best_first_not_track_order", K=4, params=dict(iou=(1, 10)),
         frames=[[(20, 0, 40, 10), (32, 0, 52, 10)], [(8, 0, 28, 10), (30, 0, 50, 10)]], want=[[0, 1], [0, 1]], flags=0),
]
BY_NAME = {c["name"]: c for c in CASES}
CASE_NAMES = [c["name"] for c in CASES]


def random_video(rng, T=None, K=None):
    """A small video of boxes that drift, vanish and come back on a coarse lattice (ties and exact thresholds are common; a box that drifts below 0 is a bad one), with now
    and then an empty box and a count that is not the number of boxes: (frames, K, n, params)."""
    T, K = int(rng.integers(1, 13)) if T is None else T, int(rng.integers(1, 9)) if K is None else K
    step = int(rng.choice([1, 5]))
    cars = [dict(x=int(rng.integers(0, 12)) * step, y=int(rng.integers(0, 4)) * step, w=int(rng.integers(2, 7)) * step, h=int(rng.integers(2, 5)) * step,
                 vx=int(rng.integers(-1, 2)) * step, vy=int(rng.integers(-1, 2)) * step) for _ in range(int(rng.integers(1, K + 3)))]
    frames, n = [], []
    for _ in range(T):
        fr = []
        for c in cars:
            c["x"] += c["vx"]
            c["y"] += c["vy"]
            if rng.random() < 0.75:
                fr.append((c["x"], c["y"], c["x"] + c["w"], c["y"] + c["h"]))
        if rng.random() < 0.1:
            fr.append((3, 3, 3, 9))
        order = rng.permutation(len(fr))
        fr = [fr[i] for i in order][:K]
        frames.append(fr)
        n.append(len(fr) if rng.random() < 0.9 else int(rng.integers(-2, K + 4)))
    params = dict(iou=[(3, 10), (1, 3), (1, 2), (1, 1024), (1, 1)][int(rng.integers(0, 5))], max_gap=int(rng.integers(0, 4)), predict=int(rng.integers(0, 2)),
                  max_tracks=int(rng.choice([3, 16, 64])))
    return frames, K, n, params
