"""numpy restatement of tmi_ba_match_features_cascade (theia_mi355_ba.h, steps 1 to 8) in fp32, written from the
reference's LOOP (cascade_hasher.cc:206-276): the candidate list in group order with the buckets filled in ascending
index, a `used` flag, the Hamming bins in insertion order, the walk that stops once it holds more than ten.  The key
formulation of step 4 is NOT used here; tests/test_cascade_matching_cpu.py states it separately and compares.  Beside
it a float64 evaluation of every projection and every decision with their margins, and the inputs of the device tests
(tests/test_gpu_cascade_matching.py)."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from matching_model import distances, nearest_two  # noqa: E402,F401
from theiasfm_amd import synth  # noqa: E402

CODE_BITS, GROUPS, GROUP_BITS, PROJ_ROWS = 128, 6, 10, 188
TOP = 10  # kNumTopCandidates
MARGIN = 1e-4  # of a distance decision: (D + 2) 2^-24 = 7.9e-6 at D = 130 bounds the fp32 sum's relative error
BIT_MARGIN = 1e-4  # of a hash bit, |sum P t| / sum |P t|: the fp32 sum is within (D + 2) 2^-24 of sum |P t|
DEFAULTS = dict(use_lowes_ratio=True, lowes_ratio=0.8, keep_only_symmetric_matches=True, min_num_feature_matches=30)


def mean(x):
    """Step 1: m = 0; m = m + x[i] for ascending i; m / (float)N."""
    m = np.zeros(x.shape[1], np.float32)
    for i in range(x.shape[0]):
        m = m + x[i]
    return (m / np.float32(x.shape[0])).astype(np.float32)


def project(x, proj):
    """Step 2, the sums: acc[i, r] over ascending k of P[r][k] * (x[i][k] - m[k]), every operation in fp32."""
    t = (x - mean(x)[None, :]).astype(np.float32)
    acc = np.zeros((x.shape[0], proj.shape[0]), np.float32)
    for k in range(x.shape[1]):
        acc = acc + proj[:, k][None, :] * t[:, k][:, None]
    return acc


def hash_image(x, proj):
    """(bits [N, 128] bool, bucket ids [N, 6] int) of one image; an empty image has neither."""
    x = np.asarray(x, np.float32)
    if x.shape[0] == 0:
        return np.zeros((0, CODE_BITS), bool), np.zeros((0, GROUPS), np.int64)
    bit = project(x, np.asarray(proj, np.float32)) > 0
    ids = np.zeros((x.shape[0], GROUPS), np.int64)
    for g in range(GROUPS):
        for k in range(GROUP_BITS):
            ids[:, g] = (ids[:, g] << 1) + bit[:, CODE_BITS + GROUP_BITS * g + k]
    return bit[:, :CODE_BITS], ids


def pack_code(bits):
    """[N, 4] uint32: code bit j is bit j % 32 of word j / 32."""
    w = np.zeros((bits.shape[0], 4), np.uint32)
    for j in range(CODE_BITS):
        w[:, j // 32] |= bits[:, j].astype(np.uint32) << np.uint32(j % 32)
    return w


def build_buckets(ids):
    """BuildBuckets: buckets[g][id] lists the rows in ascending index."""
    buckets = [dict() for _ in range(GROUPS)]
    for g in range(GROUPS):
        for j in range(ids.shape[0]):
            buckets[g].setdefault(int(ids[j, g]), []).append(j)
    return buckets


def shortlist_loop(code1_i, ids1_i, code2, buckets2):
    """The reference's walk for one row: (total, the shortlisted columns in the walk's order)."""
    candidates = []
    for g in range(GROUPS):
        candidates.extend(buckets2[g].get(int(ids1_i[g]), []))
    if len(candidates) <= TOP:
        return len(candidates), []
    used = set()
    bins = [[] for _ in range(CODE_BITS + 1)]
    for c in candidates:
        if c in used:
            continue
        used.add(c)
        bins[int(np.count_nonzero(code1_i != code2[c]))].append(c)
    out = []
    for b in bins:
        for c in b:
            out.append(c)
            if len(out) > TOP:
                break
        if len(out) > TOP:
            break
    return len(candidates), out


def match_direction(a, b, hash_a, hash_b, buckets_b, lowes_ratio_or_none):
    """MatchImages for the rows of a against b: best_i (-1: no match), best_d, second_d, passed, total per row, the
    number of exact distances, the shortlists."""
    n = a.shape[0]
    best_i = np.full(n, -1, np.int64)
    best_d = np.full(n, np.inf, np.float32)
    second_d = np.full(n, np.inf, np.float32)
    passed = np.zeros(n, bool)
    totals = np.zeros(n, np.int64)
    lists = [[] for _ in range(n)]
    if n == 0 or b.shape[0] == 0:
        return dict(best_i=best_i, best_d=best_d, second_d=second_d, passed=passed, totals=totals, lists=lists,
                    skipped=0, examined=0, evaluations=0)
    sq = float(np.float32(lowes_ratio_or_none)) ** 2 if lowes_ratio_or_none is not None else 1.0
    skipped = examined = evaluations = 0
    for i in range(n):
        total, cols = shortlist_loop(hash_a[0][i], hash_a[1][i], hash_b[0], buckets_b)
        totals[i] = total
        if not cols:
            skipped += 1
            continue
        examined += total
        evaluations += len(cols)
        lists[i] = cols
        d = distances(a[i][None, :], b[cols])[0]
        pairs = sorted(zip(d.tolist(), cols))  # std::pair<float, int>'s operator<
        best_d[i], best_i[i], second_d[i] = np.float32(pairs[0][0]), pairs[0][1], np.float32(pairs[1][0])
        passed[i] = not (float(best_d[i]) > float(second_d[i]) * sq)
    return dict(best_i=best_i, best_d=best_d, second_d=second_d, passed=passed, totals=totals, lists=lists,
                skipped=skipped, examined=examined, evaluations=evaluations)


def match_batch(image_begin, descriptors, projections, pair_image1, pair_image2, use_lowes_ratio=True,
                lowes_ratio=0.8, keep_only_symmetric_matches=True, min_num_feature_matches=30):
    """The whole call: the arrays of lib.match_features_cascade and its three counters."""
    num_images = len(image_begin) - 1
    desc = np.asarray(descriptors, np.float32)
    imgs = [desc[image_begin[m]:image_begin[m + 1]] for m in range(num_images)]
    hashes = [hash_image(x, projections) for x in imgs]
    buckets = [build_buckets(h[1]) for h in hashes]
    ratio = lowes_ratio if use_lowes_ratio else None
    status, nfwd, begin, f1, f2, dist = [], [], [0], [], [], []
    skipped = examined = evaluations = 0
    memo = {}

    def direction(r, c):
        if (r, c) not in memo:
            memo[(r, c)] = match_direction(imgs[r], imgs[c], hashes[r], hashes[c], buckets[c], ratio)
        return memo[(r, c)]

    for p in range(len(pair_image1)):
        i1, i2 = int(pair_image1[p]), int(pair_image2[p])
        fwd = direction(i1, i2)
        parts = [fwd]
        keep = fwd["passed"].copy()
        num_forward = int(keep.sum())
        if keep_only_symmetric_matches:
            rev = direction(i2, i1)  # computed whatever the forward count: nothing of it is visible on failure
            parts.append(rev)
            for i in np.nonzero(fwd["passed"])[0]:
                j = fwd["best_i"][i]
                keep[i] = rev["passed"][j] and rev["best_i"][j] == i
        for part in parts:
            skipped += part["skipped"]
            examined += part["examined"]
            evaluations += part["evaluations"]
        ok = num_forward >= min_num_feature_matches and int(keep.sum()) >= min_num_feature_matches
        rows = np.nonzero(keep)[0] if ok else np.zeros(0, np.int64)
        status.append(0 if ok else 1)
        nfwd.append(num_forward)
        begin.append(begin[-1] + rows.shape[0])
        f1.append(rows)
        f2.append(fwd["best_i"][rows])
        dist.append(fwd["best_d"][rows])
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)  # noqa: E731
    code = np.concatenate([pack_code(h[0]) for h in hashes]) if hashes else np.zeros((0, 4), np.uint32)
    ids = np.concatenate([h[1] for h in hashes]).astype(np.uint16) if hashes else np.zeros((0, 6), np.uint16)
    return dict(pair_status=np.asarray(status, np.int8), pair_num_forward=np.asarray(nfwd, np.int32),
                pair_match_begin=np.asarray(begin, np.int64), feature1=cat(f1, np.int32), feature2=cat(f2, np.int32),
                distance=cat(dist, np.float32), image_hash=code, image_bucket_ids=ids, rows_skipped=skipped,
                candidates_examined=examined, distance_evaluations=evaluations, directions=memo)


# ---- float64: the margins of the bits and of the decisions ---------------------------------------
def bit_margins(x, proj):
    """Per (row, projection row) in float64: |sum P t| / sum |P t| with the float64 mean (1 where the denominator is
    0 and the row is alone: every t is 0 in every arithmetic), and the float64 bit."""
    x = np.asarray(x, np.float64)
    p = np.asarray(proj, np.float64)
    t = x - x.mean(axis=0)[None, :]
    s = t @ p.T
    den = np.abs(t) @ np.abs(p).T
    with np.errstate(invalid="ignore", divide="ignore"):
        margin = np.where(den > 0, np.abs(s) / den, 1.0)
    return margin, s > 0


def decision_margins(a, b, cols, lowes_ratio_or_none):
    """For one row and its shortlist in float64: the relative gap of best to second, (d1 - d0) / d1, and of d0 to
    sq d1; a zero denominator gives 0."""
    d = distances(a[None, :], b[cols], np.float64)[0]
    o = np.lexsort((np.asarray(cols), d))
    d0, d1 = d[o[0]], d[o[1]]
    sq = float(np.float32(lowes_ratio_or_none)) ** 2 if lowes_ratio_or_none is not None else 1.0
    gap_best = (d1 - d0) / d1 if d1 > 0 else 0.0
    gap_ratio = abs(d0 - sq * d1) / (sq * d1) if d1 > 0 else 0.0
    return int(np.asarray(cols)[o[0]]), gap_best, gap_ratio, not (d0 > d1 * sq)


# ---- the inputs of the device tests ----------------------------------------------------------------
def _pairs(pairs):
    p = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    return p[:, 0].copy(), p[:, 1].copy()


POOLED = {  # name: (dim, pool, (N1, N2), noise, data seed)
    "pooled-d16": (16, 4, (70, 65), 0.1, 1),
    "pooled-d32": (32, 6, (96, 120), 0.05, 1),
    "pooled-d128": (128, 8, (130, 200), 0.02, 1),
}
PROJECTION_SEED = 7


@functools.lru_cache(maxsize=None)
def pooled_case(name):
    """Rows drawn from a small pool of scene descriptors plus noise: random descriptors at these sizes would leave
    every one of the 1024 buckets of a group empty or alone."""
    dim, pool, n, noise, seed = POOLED[name]
    begin, desc, _ = synth.make_matching_batch(2, n, dim, seed=seed, match_share=1.0, noise=noise, pool_size=pool)
    p1, p2 = _pairs([(0, 1), (1, 0), (0, 0)])
    return dict(name=name, image_begin=begin, descriptors=desc, projections=synth.cascade_projections(dim, PROJECTION_SEED),
                pair_image1=p1, pair_image2=p2)


@functools.lru_cache(maxsize=None)
def long_bucket_case():
    """Image 1 holds 150 noisy copies of ONE scene descriptor among 40 others with noise so small that most copies
    share all six buckets: a bucket of more than 64 rows, walked in strides against the running eleven."""
    dim = 32
    rng = np.random.default_rng(3)
    pool = rng.normal(size=(5, dim))
    pool /= np.linalg.norm(pool, axis=1, keepdims=True)
    a = pool[rng.integers(0, 5, 40)] + 0.02 * rng.normal(size=(40, dim))
    which = np.concatenate([np.zeros(150, np.int64), rng.integers(1, 5, 40)])
    b = pool[which] + 0.004 * rng.normal(size=(190, dim))
    b = b[rng.permutation(190)]
    desc = np.concatenate([a, b]).astype(np.float32)
    p1, p2 = _pairs([(0, 1), (1, 0)])
    return dict(name="long-bucket", image_begin=np.asarray([0, 40, 230], np.int64), descriptors=desc,
                projections=synth.cascade_projections(dim, PROJECTION_SEED), pair_image1=p1, pair_image2=p2)


@functools.lru_cache(maxsize=None)
def tiny_case():
    """Images of 0, 1 and 2 rows beside one of 40, and pairs of an image with itself."""
    dim = 16
    begin, desc, _ = synth.make_matching_batch(4, (0, 1, 2, 40), dim, seed=5, match_share=1.0, noise=0.05, pool_size=2)
    p1, p2 = _pairs([(0, 3), (3, 0), (0, 0), (1, 3), (3, 1), (1, 1), (2, 3), (3, 2), (2, 2), (3, 3), (1, 2)])
    return dict(name="tiny", image_begin=begin, descriptors=desc, projections=synth.cascade_projections(dim, PROJECTION_SEED),
                pair_image1=p1, pair_image2=p2)


@functools.lru_cache(maxsize=None)
def zero_secondary_case():
    """All-zero secondary projection and 2 <= N2 <= 11: every column is a candidate of every group (total = 6 N2 > 10)
    and all of them are shortlisted, so the call is the exact matcher."""
    dim = 24
    begin, desc, _ = synth.make_matching_batch(4, (37, 11, 2, 7), dim, seed=9, match_share=1.0, noise=0.05, pool_size=16)
    p1, p2 = _pairs([(0, 1), (0, 2), (0, 3), (1, 3), (3, 1), (2, 2)])
    return dict(name="zero-secondary", image_begin=begin, descriptors=desc,
                projections=synth.cascade_projections(dim, PROJECTION_SEED, zero_secondary=True), pair_image1=p1,
                pair_image2=p2)


def gpu_cases():
    return [pooled_case(n) for n in POOLED] + [long_bucket_case(), tiny_case(), zero_secondary_case()]


def case_args(case):
    return case["image_begin"], case["descriptors"], case["projections"], case["pair_image1"], case["pair_image2"]


@functools.lru_cache(maxsize=None)
def _model_cached(name, key):
    case = next(c for c in gpu_cases() if c["name"] == name)
    return match_batch(*case_args(case), **dict(key))


def model(case, **options):
    """match_batch of a case, computed once per (case, options) and shared: treat the result as read-only."""
    o = dict(DEFAULTS)
    o.update(options)
    return _model_cached(case["name"], tuple(sorted(o.items())))
