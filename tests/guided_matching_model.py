"""Pure-Python / numpy restatement of tmi_ba_guided_epipolar_match (theia_mi355_ba.h, steps a to f), written from the
header: the fp64 geometry in Python floats (every + - * / sqrt rounded on its own, never contracted), the fp32
distances through tests/matching_model.py.  Candidate sets are Python sets, groups are built by sorting tuples: nothing
is shared with the device's sorts, bitmaps or butterflies.

Every decision the fp64 geometry feeds is counted by Decisions with its distance from its boundary.  A risky one (too
close to call) is turned to see whether it reaches an output: those of the walks on the spot, through the cell the
other outcome would take; the others by `flip`, which runs the pair with that one decision inverted
(tests/test_guided_matching_cpu.py demands that none on the device tests' inputs changes an output)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import matching_model as mm  # noqa: E402

MARGIN = 1e-9  # relative; the fp64 chains here are a few operations long (errors of a few 2^-53)
RATIO_MARGIN = mm.MARGIN  # the ratio test compares fp32 sums: the exact matcher's margin
DEFAULTS = dict(guided_matching_max_distance_pixels=2.0, lowes_ratio=0.8, min_num_candidates=50, seed=0)
MASK64 = (1 << 64) - 1


def splitmix64_word(seed, c):
    z = (seed + (c + 1) * 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def fill_draw(seed, stream, group, t, n2):
    u = (float(splitmix64_word(seed, 64 * ((stream << 32) + group) + t) >> 11) + 0.5) * (1.0 / 9007199254740992.0)
    return min(int(u * float(n2)), n2 - 1)


def _small_dyadic(*values):
    """Multiples of 2^-8 below 2^17: their differences, squares and sums of two squares are exact in fp64."""
    return all(math.isfinite(v) and abs(v) < 131072.0 and v * 256.0 == math.floor(v * 256.0) for v in values)


class Decisions:
    """take(kind, outcome, gap, exact): `gap` is the distance of the decision from its boundary; `exact` says the
    compared values were computed without rounding.  Risky: 0 < gap < margin, or a tie (gap 0) that is not exact --
    the decisions a different rounding could turn.  flagged: the risky ones outside the walks, to be flipped."""

    def __init__(self, flip=None):
        self.count = 0
        self.flagged = []  # (id, kind, gap)
        self.ties = 0
        self.walk_risky = {}     # kind -> risky decisions of the walks
        self.walk_affecting = []  # (group, step, kind): a risky decision whose alternative changes the candidate set
        self.flip = flip

    def risky(self, kind, gap, exact=False, margin=MARGIN):
        """Counts a decision of the walk (its alternatives are examined on the spot, not by a flip)."""
        self.count += 1
        bad = (gap == 0.0 and not exact) or (0.0 < gap < margin)
        if bad:
            self.walk_risky[kind] = self.walk_risky.get(kind, 0) + 1
        return bad

    def take(self, kind, outcome, gap, exact=False, margin=MARGIN):
        i = self.count
        self.count += 1
        if (gap == 0.0 and not exact) or (gap != 0.0 and not (gap >= margin)):
            self.ties += 1 if gap == 0.0 else 0
            self.flagged.append((i, kind, gap))
        return (not outcome) if self.flip == i else outcome


def _gap(a, b):
    if not (math.isfinite(a) and math.isfinite(b)):
        return math.inf  # a NaN or an infinity fails its test whatever the rounding
    return abs(a - b) / max(1.0, abs(a), abs(b))


def _axis_cell(v, o, c):
    """One axis of a cell centre: (centre, alternative centre, gap, exact).  The alternative is the centre of the
    neighbouring cell on the side of the nearer border, `gap` the distance of (v - o) / (2 c) from that border in
    cells; exact: the quotient is computed without rounding.  For a small dyadic c the centre is a sum of small
    multiples of c, so it and its truncation are exact whatever the rounding of the quotient."""
    q = (v - o) / (2.0 * c)
    f = math.floor(q)
    centre = int(((f * 2.0) * c + c) + o)
    other = f - 1.0 if q - f < 0.5 else f + 1.0
    alt = int(((other * 2.0) * c + c) + o)
    return centre, alt, min(q - f, f + 1.0 - q), _small_dyadic(v, o, c) and c in (0.5, 1.0, 2.0, 4.0, 8.0)


def cell_centre(x, y, grid, c):
    return (_axis_cell(x, c if grid & 1 else 0.0, c)[0], _axis_cell(y, c if grid & 2 else 0.0, c)[0])


def _cell_with_alternatives(x, y, grid, c, D, kind):
    """The centre of (x, y) in `grid`, and the centres a different rounding of a risky floor would give."""
    ax = _axis_cell(x, c if grid & 1 else 0.0, c)
    ay = _axis_cell(y, c if grid & 2 else 0.0, c)
    alts = []
    if D.risky(kind, ax[2], ax[3]):
        alts.append((ax[1], ay[0]))
    if D.risky(kind, ay[2], ay[3]):
        alts.append((ax[0], ay[1]))
    return (ax[0], ay[0]), alts


def _closest(sx, sy, centres):
    """(best grid, best distance, runner-up grid, runner-up distance) with strict < in grid order."""
    best, best_grid, runner, runner_grid = math.inf, -1, math.inf, -1
    for grid, (cx, cy) in enumerate(centres):
        ux, uy = float(cx) - sx, float(cy) - sy
        d = ux * ux + uy * uy
        if d < best:
            runner, runner_grid = best, best_grid
            best, best_grid = d, grid
        elif d < runner:
            runner, runner_grid = d, grid
    return best_grid, best, runner_grid, runner


def fundamental_line(F, x, y):
    l0 = (F[0] * x + F[1] * y) + F[2]
    l1 = (F[3] * x + F[4] * y) + F[5]
    l2 = (F[6] * x + F[7] * y) + F[8]
    n = math.sqrt(l0 * l0 + l1 * l1)
    if n == 0.0 or not math.isfinite(n):
        return (math.nan,) * 3 if n == 0.0 else (l0 / n, l1 / n, l2 / n)
    return l0 / n, l1 / n, l2 / n


def _div(a, b):
    """IEEE a / b."""
    if b == 0.0:
        if a == 0.0 or math.isnan(a):
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def line_endpoints(line, box, D):
    """Step b after the line: the two endpoints [(x, y), (x, y)] or None; the code's coordinates truncated."""
    l0, l1, l2 = line
    tlx, tly, brx, bry = box
    found = []

    def test(v, lo, hi, point):
        a = D.take("endpoint-low", v >= lo, _gap(v, lo))
        b = D.take("endpoint-high", v <= hi, _gap(v, hi))
        if a and b:
            found.append(point)

    v = _div(-(l2 + l0 * tlx), l1)
    test(v, tly, bry, (tlx, v, False, True))
    v = _div(-(l2 + l1 * tly), l0)
    test(v, tlx, brx, (v, tly, True, False))
    v = _div(-(l2 + l0 * brx), l1)
    test(v, tly, bry, (brx, v, False, True))
    v = _div(-(l2 + l1 * bry), l0)
    test(v, tlx, brx, (v, bry, True, False))
    if len(found) != 2:
        return None
    coords = []
    for x, y, x_computed, y_computed in found:
        for v, computed in ((x, x_computed), (y, y_computed)):
            t = float(math.trunc(v))
            # a box coordinate is copied, not computed: its truncation is the same on every machine
            gap = abs(v - round(v)) if computed else math.inf
            if computed and v == round(v) and _small_dyadic(*line) and _small_dyadic(*box):
                gap = math.inf  # e.g. an exactly horizontal line: the intersection is the keypoint's own coordinate
            if not D.take("truncation", True, gap):  # flipped: the integer on the other side
                t = float(round(v)) if float(round(v)) != t else t - 1.0
            if not (0.0 <= t <= 65535.0):
                return None
            coords.append(int(t))
    return coords


def guided_pair(desc1, keys1, desc2, keys2, F, match1, match2, stream=0, flip=None,
                guided_matching_max_distance_pixels=2.0, lowes_ratio=0.8, min_num_candidates=50, seed=0):
    """One pair: dict(status, feature_group [N1], group_endpoints [G, 4], group_num_candidates [G], group_features,
    group_candidates, feature1, feature2, distance, decisions)."""
    c = float(guided_matching_max_distance_pixels)
    D = Decisions(flip)
    n1, n2 = len(keys1), len(keys2)
    F = [float(v) for v in np.asarray(F, np.float64).reshape(9)]
    matched1 = set(int(i) for i in match1)
    matched2 = set(int(j) for j in match2)
    un1 = [i for i in range(n1) if i not in matched1]
    un2 = [j for j in range(n2) if j not in matched2]
    out = dict(status=1, feature_group=np.full(n1, -1, np.int32), group_endpoints=np.zeros((0, 4)),
               group_num_candidates=np.zeros(0, np.int32), group_features=[], group_candidates=[],
               feature1=np.zeros(0, np.int32), feature2=np.zeros(0, np.int32), distance=np.zeros(0, np.float32),
               decisions=D)
    if not un1 or not un2:
        return out
    out["status"] = 0
    xs = [float(keys2[j][0]) for j in un2]
    ys = [float(keys2[j][1]) for j in un2]
    box = (min(xs), min(ys), max(xs), max(ys))
    # b
    coded = []
    for i in un1:
        line = fundamental_line(F, float(keys1[i][0]), float(keys1[i][1]))
        e = line_endpoints(line, box, D)
        if e is not None:
            coded.append(((e[0] << 48) | (e[1] << 32) | (e[2] << 16) | e[3], i))
    coded.sort()
    # c
    groups = []  # [E0x, E0y, E1x, E1y, features]
    sq_max = c * c
    for code, i in coded:
        x1, y1 = float((code >> 48) & 0xFFFF), float((code >> 32) & 0xFFFF)
        x2, y2 = float((code >> 16) & 0xFFFF), float(code & 0xFFFF)
        fresh = not groups
        if not fresh:
            g = groups[-1]
            dx, dy = g[0] - x1, g[1] - y1
            d2 = dx * dx + dy * dy
            fresh = D.take("group-split", d2 > sq_max, abs(d2 - sq_max) / sq_max, _small_dyadic(g[0], g[1], x1, y1, c))
        if fresh:
            groups.append([x1, y1, x2, y2, []])
        g = groups[-1]
        g[4].append(i)
        w = 1.0 / float(len(g[4]))
        g[0] = (1.0 - w) * g[0] + w * x1
        g[1] = (1.0 - w) * g[1] + w * y1
        g[2] = (1.0 - w) * g[2] + w * x2
        g[3] = (1.0 - w) * g[3] + w * y2
    # d
    cells = [dict() for _ in range(4)]
    for j in un2:
        for grid in range(4):
            x, y = float(keys2[j][0]), float(keys2[j][1])
            ax = _axis_cell(x, c if grid & 1 else 0.0, c)
            ay = _axis_cell(y, c if grid & 2 else 0.0, c)
            cx = ax[0] if D.take("cell-of-feature", True, ax[2], ax[3]) else ax[1]
            cy = ay[0] if D.take("cell-of-feature", True, ay[2], ay[3]) else ay[1]
            cells[grid].setdefault((cx, cy), []).append(j)
    # e, f
    ratio_sq = float(lowes_ratio) * float(lowes_ratio)
    desc1 = np.asarray(desc1, np.float32)
    desc2 = np.asarray(desc2, np.float32)
    f1, f2, dist, ncand = [], [], [], []
    for gi, (E0x, E0y, E1x, E1y, feats) in enumerate(groups):
        for i in feats:
            out["feature_group"][i] = gi
        dx, dy = E1x - E0x, E1y - E0y
        steps_real = math.sqrt(dx * dx + dy * dy) / c
        num_steps = int(steps_real)
        if not D.take("num-steps", True, abs(steps_real - round(steps_real)),
                      _small_dyadic(c) and ((dy == 0.0 and _small_dyadic(E0x, E1x)) or
                                            (dx == 0.0 and _small_dyadic(E0y, E1y)))):  # flipped: the other count
            num_steps = int(round(steps_real)) if int(round(steps_real)) != num_steps else num_steps - 1
        cand = set()
        if num_steps > 0:
            delta_x, delta_y = (E0x - E1x) / float(num_steps), (E0y - E1y) / float(num_steps)
            sx, sy = E1x, E1y
            chosen, doubtful = [], []  # per step the cell taken; (step, kind, the cell a risky decision could give)
            for step in range(num_steps):
                sx = sx + delta_x
                sy = sy + delta_y
                centres, alts = [], []
                for grid in range(4):
                    centre, a = _cell_with_alternatives(sx, sy, grid, c, D, "cell-of-sample")
                    centres.append(centre)
                    alts.append(a)
                best_grid, best, runner_grid, runner = _closest(sx, sy, centres)
                take = (best_grid, centres[best_grid])
                # a tie is exact when the two centres differ only along axes whose sample coordinate is exact
                tie_exact = runner_grid >= 0 and all(
                    centres[best_grid][k] == centres[runner_grid][k] or _small_dyadic((sx, sy)[k], c) for k in (0, 1))
                if runner_grid >= 0 and D.risky("closest-centre", abs(runner - best) / max(1.0, best), tie_exact):
                    doubtful.append((step, "closest-centre", (runner_grid, centres[runner_grid])))
                for grid in range(4):
                    for alt in alts[grid]:
                        other = list(centres)
                        other[grid] = alt
                        g2 = _closest(sx, sy, other)[0]
                        if (g2, other[g2]) != take:
                            doubtful.append((step, "cell-of-sample", (g2, other[g2])))
                chosen.append(take)
                cand.update(cells[take[0]].get(take[1], ()))
            if doubtful:
                uses = {}
                for grid, centre in chosen:
                    for j in cells[grid].get(centre, ()):
                        uses[j] = uses.get(j, 0) + 1
                for step, kind, (grid, centre) in doubtful:
                    new = set(cells[grid].get(centre, ()))
                    old = cells[chosen[step][0]].get(chosen[step][1], ())
                    if (new - cand) or any(uses[j] == 1 and j not in new for j in old):
                        D.walk_affecting.append((gi, step, kind))
        for t in range(len(cand), int(min_num_candidates)):
            cand.add(fill_draw(int(seed), int(stream), gi, t, n2))
        ncand.append(len(cand))
        cols = sorted(cand)
        out["group_candidates"].append(cols)
        out["group_features"].append(list(feats))
        if len(cols) < 2:
            continue
        d = mm.distances(desc1[feats], desc2[cols])
        bd, bi, sd = mm.nearest_two(d)
        for q, i in enumerate(feats):
            d0, d1 = float(bd[q]), float(sd[q])
            rhs = d1 * ratio_sq
            ok = D.take("ratio", d0 < rhs, abs(d0 - rhs) / rhs if rhs > 0 else 0.0, margin=RATIO_MARGIN)
            if d1 > 0:  # best against second best: which candidate wins
                D.take("nearest", True, (d1 - d0) / d1, exact=False, margin=RATIO_MARGIN)
            if ok:
                f1.append(i)
                f2.append(cols[int(bi[q])])
                dist.append(bd[q])
    out.update(group_endpoints=np.asarray([g[:4] for g in groups], np.float64).reshape(-1, 4),
               group_num_candidates=np.asarray(ncand, np.int32), feature1=np.asarray(f1, np.int32),
               feature2=np.asarray(f2, np.int32), distance=np.asarray(dist, np.float32))
    return out


def guided_batch(image_begin, descriptors, keypoints, pair_image1, pair_image2, fundamental_matrix, pair_match_begin,
                 match_feature1, match_feature2, pair_mask=None, pair_stream=None, **options):
    """The whole call: the arrays of lib.guided_epipolar_match(..., want_groups=True) and `pairs`, the per-pair dicts
    (None for a masked pair)."""
    P = len(pair_image1)
    F = np.asarray(fundamental_matrix, np.float64).reshape(P, 9)
    status, ngroups, begin, rows = [], [], [0], [0]
    f1, f2, dist, fg, ge, gn, pairs = [], [], [], [], [], [], []
    for p in range(P):
        i1, i2 = int(pair_image1[p]), int(pair_image2[p])
        a, b = slice(image_begin[i1], image_begin[i1 + 1]), slice(image_begin[i2], image_begin[i2 + 1])
        n1 = a.stop - a.start
        rows.append(rows[-1] + n1)
        g_e, g_n = np.zeros((n1, 4)), np.zeros(n1, np.int32)
        if pair_mask is not None and not pair_mask[p]:
            r = None
            status.append(-1)
            ngroups.append(0)
            fg.append(np.full(n1, -1, np.int32))
        else:
            m = slice(pair_match_begin[p], pair_match_begin[p + 1])
            r = guided_pair(descriptors[a], keypoints[a], descriptors[b], keypoints[b], F[p], match_feature1[m],
                            match_feature2[m], stream=int(pair_stream[p]) if pair_stream is not None else p, **options)
            G = len(r["group_num_candidates"])
            status.append(r["status"])
            ngroups.append(G)
            fg.append(r["feature_group"])
            g_e[:G] = r["group_endpoints"]
            g_n[:G] = r["group_num_candidates"]
            f1.append(r["feature1"])
            f2.append(r["feature2"])
            dist.append(r["distance"])
        pairs.append(r)
        ge.append(g_e)
        gn.append(g_n)
        begin.append(begin[-1] + (0 if r is None else len(r["feature1"])))
    cat = lambda xs, t, shape=(0,): np.concatenate(xs).astype(t) if xs else np.zeros(shape, t)  # noqa: E731
    return dict(pair_status=np.asarray(status, np.int8), pair_num_groups=np.asarray(ngroups, np.int32),
                pair_added_begin=np.asarray(begin, np.int64), feature1=cat(f1, np.int32), feature2=cat(f2, np.int32),
                distance=cat(dist, np.float32), pair_row=np.asarray(rows, np.int64), feature_group=cat(fg, np.int32),
                group_endpoints=cat(ge, np.float64, (0, 4)), group_num_candidates=cat(gn, np.int32), pairs=pairs)


# ---- F from two cameras, as theia::GuidedEpipolarMatcher forms it ---------------------------------
def fundamental_from_projections(pmatrix1, pmatrix2):
    """FundamentalMatrixFromProjectionMatrices (fundamental_matrix_util.cc:222-241): F[r][c] = the determinant of the
    rows index1[c], index2[c] of pmatrix2 over the rows index1[r], index2[r] of pmatrix1.  The matcher calls it as
    (P of camera 2, P of camera 1), which makes F map a point of image 1 to its line in image 2."""
    P1 = np.asarray(pmatrix1, np.float64).reshape(3, 4)
    P2 = np.asarray(pmatrix2, np.float64).reshape(3, 4)
    index1 = (1, 2, 0)
    index2 = (2, 0, 1)
    F = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            F[r, c] = np.linalg.det(np.stack([P2[index1[c]], P2[index2[c]], P1[index1[r]], P1[index2[r]]]))
    return F
