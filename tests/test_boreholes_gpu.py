"""Borehole logs on the device (csrc/gbp_boreholes.h k_borehole_score through gbp_borehole_score; geobipy_amd.boreholes score /
log_predictive and the ``boreholes=`` keyword of geobipy_amd.sections).

The score is held to the rule ``boreholes.score_reference`` evaluated in long double -- never to device output -- within a bound that
is a priori: it is built from the rule's own terms in long double (``terms=True``), the sizes of the case and the accuracy of the
device's log10 / exp / log, not from what the device returns.  With U = 2^-52, K the layer capacity, C the classes, a_max the largest
|log10 sigma| of the sounding, z = |bottom| + |shift| the size of the numbers the interval's ends are rounded at and h = b' - t':

  the layer values            a device log10 within 4 U relative (what test_families_gpu.py assumes of the same expression):
                              |da| <= ea = 4 U a_max.
  the segments                t' and b' are one rounded sum each, off by at most U z / 2; this moves the interval's two ends over values
                              of at most ``peak``, the largest |value| among the interval's segments in the long-double rule
                              (``peaks`` of ``score_reference``; an end rounded across an interface lets in a sliver of the next
                              layer, which is one of those segments), so the mean moves by at most U (z / h) peak in the numerator
                              and as much through h: 2 U (z / h) peak.  At most K + 1 products and sums and one division follow:
                              (K + 4) U V for values of size V.
  a MEASURED term             |dmean| <= em = (K + 16) U a_max + 2 U (z / h) peak (the lines above with V = a_max, and 2 ea);
                              term = -d^2 / den with den = 2 (sd^2 + var) and |d| = sqrt(|term| den) from the long-double term:
                              |dterm| <= (2 |d| em + em^2) / den + 8 U |term| (five roundings of den, d^2 and the quotient).
  a LITHOLOGY term            x = l_q(a) - l_c(a) moves by at most X = 2 (D / v_min) ea + 16 U (Q + L): the slope of l in a is at most
                              D / v_min with D = a_max + max |mu| and v_min the smallest scale^2 + var; each l is a few roundings of
                              numbers up to Q = D^2 / (2 v_min) and L = max (|ln pi| + |ln v| / 2), the device's log within 2 U.
                              exp within 2 U relative turns X into a relative error of every summand, the summands are positive
                              and the sum holds exp(0) = 1, so P = 1 / sum is off by at most rP = X + (C + 4) U relative.  Pbar
                              inherits rP, (K + 4) U of its own sum and 2 U (z / h) peak from the segments; arg = floor + (1 -
                              floor) Pbar >= (1 - floor) Pbar, so |darg| / arg <= rP + (K + 8) U + 2 U (z / h) peak / arg with 1 /
                              arg = exp(|term|) from the long-double term; a log within 2 U: |dterm| <= that + 2 U |term| + U.
  the sums                    every term is <= 0, so the partial sums are bounded by |part| and |score|:
                              |dpart| <= sum |dterm| + I U |part|,  |dscore| <= sum |dpart| + A_s U |score|.

Every case prints used / bound.  Held with ``==``: the zeros the rule prescribes, ``skipped``, identical models, a second call,
``block=1`` against one launch, and ``score`` against the ordered sum of ``part``.  The wiring is held bit for bit to
``sections(..., score=borehole_score)``."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from geobipy_amd import _lib, boreholes, sections
from test_boreholes import BORE_ROW, LITH_CLASSES, planted_log
from test_families_gpu import _to_device
from test_spatial_sections import S_LINES, Z1_LINES, planted_lines

U = 2.0 ** -52
CLASSES = ([-2.5, -1.0, 0.5], [0.2, 0.4, 0.3], [0.5, 0.3, 0.2])


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _numpy(d):
    return {n: (v.cpu().numpy() if torch.is_tensor(v) else v) for n, v in d.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _case(S, n, K, n_int, n_att, kind, seed):
    """An ensemble of S soundings with n + 2 slots (k from 1 to K, a half-space and a full model among them, slot 1 a copy of slot 0,
    the last slot empty), a row list of n entries that names -1 and the empty slot where n allows, n_used < n on every third sounding;
    three boreholes of ``n_int`` intervals each between 0 and about 110 m with gaps (the second one has none when n_int is 0 or 1),
    ``kind`` measured, lithology or mixed; some interfaces are set exactly on interval ends; ``n_att`` attachments on sounding 0 and 0,
    1 or 3 on the others in turn, with shifts of both signs: -7 m cuts or skips the first intervals."""
    rng = np.random.default_rng(seed)
    ns = n + 2
    k = np.zeros((S, ns), dtype=np.int32)
    edges, sigma = np.full((S, ns, K), np.inf), np.full((S, ns, K), np.nan)
    tops, bottoms, values, sds, cls, ptr = [], [], [], [], [], [0]
    for b in range(3):
        m = n_int if (b != 1 or n_int > 1) else 0
        cuts = np.sort(rng.uniform(0.0, 110.0, 2 * m))
        if m:
            cuts[0] = 0.0 if b == 0 else cuts[0]
        for i in range(m):
            t, bt = cuts[2 * i], cuts[2 * i + 1]
            if i % 3 == 1 and len(tops) > ptr[-1]:
                t = bottoms[-1]                                               # no gap: the interval starts where the one before ends
            if not bt > t:
                continue
            lith = kind == "lithology" or (kind == "mixed" and (i + b) % 2 == 1)
            tops.append(t), bottoms.append(bt)
            values.append(np.nan if lith else rng.uniform(-3.0, 0.5)), sds.append(np.nan if lith else rng.uniform(0.05, 0.5))
            cls.append(int(rng.integers(0, 3)) if lith else -1)
        ptr.append(len(tops))
    logs = boreholes.Logs([0.0, 1.0, 2.0], [0.0, 0.0, 0.0], None, ptr, tops, bottoms, values, sds, np.array(cls, dtype=np.int64))
    ends = np.array(tops + bottoms) if tops else np.array([10.0])
    for s in range(S):
        for q in range(ns - 1):
            kk = [1, K, min(2, K)][q] if q < 3 else int(rng.integers(1, K + 1))
            e = np.sort(rng.uniform(0.5, 130.0, kk - 1))
            if kk > 1 and q % 2 == 0:
                e[rng.integers(0, kk - 1)] = ends[rng.integers(0, ends.size)] + [0.0, 3.0, -7.0][q % 3]      # an interface on an interval's end, shifted or not
                e = np.sort(np.abs(e) + 0.25 * (e <= 0))
            k[s, q] = kk
            edges[s, q, :kk - 1] = e
            sigma[s, q, :kk] = 10.0 ** rng.uniform(-4.0, 1.0, kk)
            if kk < K:
                sigma[s, q, kk:] = -1.0                                        # entries past k are never read
        k[s, 1], edges[s, 1], sigma[s, 1] = k[s, 0], edges[s, 0], sigma[s, 0]
    rows = np.stack([rng.permutation(ns)[:n] for _ in range(S)]).astype(np.int32)
    if n >= 15:
        rows[:, 2], rows[:, 5], rows[:, 7], rows[:, 9], rows[:, 11] = ns - 1, -1, ns, 0, 1
    n_used = np.where(np.arange(S) % 3 == 2, max(1, n - 3), n).astype(np.int32)
    counts = np.array([n_att] + [[0, 1, 3][(s - 1) % 3] for s in range(1, S)])
    att_s = np.repeat(np.arange(S), counts)
    A = att_s.size
    att = dict(att_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), att_sounding=att_s.astype(np.int32),
               att_bore=(np.arange(A) % 3).astype(np.int32), att_var=np.where(np.arange(A) % 2 == 0, 0.0, rng.uniform(0.0, 0.09, A)),
               att_shift=np.array([0.0, 3.0, -7.0, -200.0])[(np.arange(A) + seed) % 4] * (np.arange(A) % 5 != 4), att_distance=np.zeros(A))
    return k, edges, sigma, rows, n_used, att, logs


def _bound(k, edges, sigma, rows, n_used, att, logs, ld, K):
    """The a-priori bound of the module's docstring for score [S, n] and part [A, n], from the long-double rule ``ld`` (terms=True)."""
    mu, sc, pr = (np.asarray(a, dtype=np.float64) for a in CLASSES)
    C = mu.size
    S, n = rows.shape
    e_part, e_score = np.zeros((att["att_bore"].size, n)), np.zeros((S, n))
    for s in range(S):
        a0, a1 = int(att["att_ptr"][s]), int(att["att_ptr"][s + 1])
        if a0 == a1:
            continue
        live = sigma[s][k[s] > 0]
        a_max = float(np.nanmax(np.abs(np.log10(np.where(live > 0, live, np.nan))))) if live.size else 0.0
        ea = 4 * U * a_max
        for a in range(a0, a1):
            b, var, shift = int(att["att_bore"][a]), float(att["att_var"][a]), float(att["att_shift"][a])
            v = sc * sc + var
            D, v_min = a_max + float(np.abs(mu).max()), float(v.min())
            X = 2 * (D / v_min) * ea + 16 * U * (D * D / (2 * v_min) + float((np.abs(np.log(pr)) + 0.5 * np.abs(np.log(v))).max()))
            rP = X + (C + 4) * U
            i0, i1 = int(logs.ptr[b]), int(logs.ptr[b + 1])
            total = np.zeros(n)
            for i in range(i0, i1):
                tp, bp = max(logs.top[i] + shift, 0.0), logs.bottom[i] + shift
                if bp <= tp:
                    continue
                t = np.abs(ld["terms"][a][i - i0].astype(np.float64))
                peak = ld["peaks"][a][i - i0].astype(np.float64)
                zh = (abs(logs.bottom[i]) + abs(shift)) / (bp - tp)
                if logs.cls[i] < 0:
                    den = 2.0 * (logs.sd[i] ** 2 + var)
                    em = (K + 16) * U * a_max + 2 * U * zh * peak
                    total += (2 * np.sqrt(t * den) * em + em * em) / den + 8 * U * t
                else:
                    total += rP + (K + 8) * U + 2 * U * zh * peak * np.exp(t) + 2 * U * t + U
            e_part[a] = total + (i1 - i0) * U * np.abs(ld["part"][a].astype(np.float64))
            e_score[s] += e_part[a]
        e_score[s] += (a1 - a0) * U * np.abs(ld["score"][s].astype(np.float64))
    return e_score, e_part


CASES = [(1, 1, 1, 1, 1, "measured"), (1, 63, 4, 2, 3, "mixed"), (5, 64, 4, 65, 1, "lithology"), (5, 65, 64, 2, 3, "mixed"), (70, 130, 4, 0, 1, "measured"),
         (70, 65, 1, 65, 3, "mixed"), (5, 130, 64, 300, 3, "mixed"), (1, 64, 64, 300, 1, "lithology"), (5, 63, 4, 65, 0, "measured"), (1, 130, 1, 1, 3, "lithology")]


@pytest.mark.parametrize("S,n,K,n_int,n_att,kind", CASES)
def test_score_against_the_long_double_rule(S, n, K, n_int, n_att, kind):
    label = "S=%d n=%d K=%d I=%d att=%d %s" % (S, n, K, n_int, n_att, kind)
    k, edges, sigma, rows, n_used, att, logs = _case(S, n, K, n_int, n_att, kind, 1000 * S + 10 * n + K + n_int)
    ens, dev = _to_device(k, edges, sigma), _dev()
    t_rows, t_nu = torch.as_tensor(rows).to(dev), torch.as_tensor(n_used).to(dev)
    got = _numpy(boreholes.score(ens, t_rows, t_nu, att, logs, classes=CLASSES))
    again = _numpy(boreholes.score(ens, t_rows, t_nu, att, logs, classes=CLASSES))
    single = _numpy(boreholes.score(ens, t_rows, t_nu, att, logs, classes=CLASSES, block=1))
    A = att["att_bore"].size
    assert got["score"].shape == (S, n) and got["part"].shape == (A, n) and got["skipped"].shape == (A,) and got["skipped"].dtype == np.int32
    for name in ("score", "part", "skipped"):                                  # a second call and block=1, bit for bit
        assert np.array_equal(got[name], again[name], equal_nan=True) and np.array_equal(got[name], single[name], equal_nan=True), (label, name)
    assert np.array_equal(_bits(got["score"]), _bits(again["score"])) and np.array_equal(_bits(got["score"]), _bits(single["score"]))
    ld = boreholes.score_reference(k, edges, sigma, rows, n_used, att, logs, classes=CLASSES, dtype=np.longdouble, terms=True)
    assert np.array_equal(got["skipped"], ld["skipped"]), label
    ns = k.shape[1]
    for s in range(S):
        a0, a1 = int(att["att_ptr"][s]), int(att["att_ptr"][s + 1])
        absent = np.array([m >= n_used[s] or not (0 <= rows[s, m] < ns) or k[s, min(max(rows[s, m], 0), ns - 1)] <= 0 for m in range(n)])
        assert np.all(_bits(got["score"][s, absent]) == 0) and np.all(_bits(got["part"][a0:a1][:, absent]) == 0), (label, s, "zeros of absent models")
        if a0 == a1:
            assert np.all(_bits(got["score"][s]) == 0), (label, s, "zeros without attachments")
        total = np.zeros(n)
        for a in range(a0, a1):
            total = total + got["part"][a]
        assert np.array_equal(_bits(got["score"][s]), _bits(total)), (label, s, "score is the ordered sum of part")
        same = np.isin(rows[s], (0, 1)) & ~absent
        if same.sum() > 1:
            assert np.unique(_bits(got["score"][s, same])).size == 1, (label, s, "identical models")
    if n_int > 0 and A >= 8:
        assert ld["skipped"].max() > 0 and ld["skipped"].min() == 0, label      # (the case holds skipped intervals, and attachments without)
    e_score, e_part = _bound(k, edges, sigma, rows, n_used, att, logs, ld, K)
    d_score = np.abs(got["score"].astype(np.longdouble) - ld["score"]).astype(np.float64)
    d_part = np.abs(got["part"].astype(np.longdouble) - ld["part"]).astype(np.float64)
    assert np.all(np.isfinite(got["score"])) and np.all(np.isfinite(ld["score"].astype(np.float64)))
    live_s, live_p = e_score > 0, e_part > 0
    used_s = float((d_score[live_s] / e_score[live_s]).max()) if live_s.any() else 0.0
    used_p = float((d_part[live_p] / e_part[live_p]).max()) if live_p.any() else 0.0
    print("%s used/bound: score %.3g part %.3g (largest |score| %.3g, largest bound %.3g)" % (label, used_s, used_p, float(np.abs(got["score"]).max()),
                                                                                           float(e_score.max())))
    assert np.all(d_score <= e_score), (label, "score", float((d_score - e_score).max()))
    assert np.all(d_part <= e_part), (label, "part", float((d_part - e_part).max()))


def test_part_and_skipped_may_be_left_out_and_the_entry_refuses_by_name():
    k, edges, sigma, rows, n_used, att, logs = _case(5, 65, 4, 2, 3, "mixed", 7)
    ens, dev = _to_device(k, edges, sigma), _dev()
    S, n, K, ns = 5, 65, 4, k.shape[1]
    A, Nb, I = att["att_bore"].size, 3, logs.n_intervals
    want = boreholes.score(ens, torch.as_tensor(rows).to(dev), torch.as_tensor(n_used).to(dev), att, logs, classes=CLASSES)
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
    t = dict(rows=up(rows, np.int32), nu=up(n_used, np.int32), aptr=up(att["att_ptr"], np.int32), abore=up(att["att_bore"], np.int32), avar=up(att["att_var"], np.float64),
             ashift=up(att["att_shift"], np.float64), bptr=up(logs.ptr, np.int32), top=up(logs.top, np.float64), bottom=up(logs.bottom, np.float64),
             value=up(logs.value, np.float64), sd=up(logs.sd, np.float64), cls=up(logs.cls, np.int32))
    score = torch.full((S, n), 7.0, dtype=torch.float64, device=dev)
    part = torch.full((A, n), 7.0, dtype=torch.float64, device=dev)
    skipped = torch.full((A,), 7, dtype=torch.int32, device=dev)
    arr = lambda v: (_lib.ctypes.c_double * 16)(*v)                            # noqa: E731
    mu, sc, ln = arr(CLASSES[0]), arr(CLASSES[1]), arr(np.log(CLASSES[2]))
    p = lambda a: None if a is None else a.data_ptr()                          # noqa: E731

    def call(S_=S, ns_=ns, K_=K, n_=n, A_=A, Nb_=Nb, I_=I, C_=3, floor=1e-6, mu_=mu, sc_=sc, ln_=ln, part_=part, skipped_=skipped, score_=score, **over):
        a = dict(t, **over)
        return lib.gbp_borehole_score(S_, ns_, K_, p(ens.k), p(ens.edges), p(ens.sigma), n_, p(a["rows"]), p(a["nu"]), A_, p(a["aptr"]), p(a["abore"]), p(a["avar"]),
                                      p(a["ashift"]), Nb_, p(a["bptr"]), I_, p(a["top"]), p(a["bottom"]), p(a["value"]), p(a["sd"]), p(a["cls"]), C_, mu_, sc_, ln_,
                                      floor, p(score_), p(part_), p(skipped_), st)

    bad_ptr, bad_bore, bad_cls, bad_bptr = t["aptr"].clone(), t["abore"].clone(), t["cls"].clone(), t["bptr"].clone()
    bad_ptr[2], bad_bore[1], bad_cls[0], bad_bptr[1] = A + 1, Nb, 3, I + 1
    for kw in (dict(S_=-1), dict(ns_=0), dict(n_=0), dict(n_=1025), dict(K_=0), dict(K_=65), dict(C_=-1), dict(C_=17), dict(A_=-1), dict(Nb_=-1), dict(I_=-1), dict(Nb_=0),
               dict(floor=0.0), dict(floor=1.0), dict(floor=float("nan")), dict(mu_=None), dict(sc_=arr([0.2, 0.0, 0.3])), dict(ln_=arr([0.0, float("inf"), 0.0])),
               dict(mu_=arr([float("nan"), 0.0, 0.0])), dict(rows=None), dict(nu=None), dict(aptr=None), dict(score_=None), dict(abore=None), dict(avar=None),
               dict(ashift=None), dict(bptr=None), dict(top=None), dict(cls=None), dict(aptr=bad_ptr), dict(abore=bad_bore), dict(cls=bad_cls), dict(bptr=bad_bptr),
               dict(A_=A - 1), dict(I_=I - 1)):
        assert call(**kw) != 0 and b"gbp_borehole_score" in lib.gbp_last_error(), kw
    torch.cuda.synchronize()
    assert bool((score == 7.0).all()) and bool((part == 7.0).all()) and bool((skipped == 7).all())      # nothing was written
    assert call(part_=None, skipped_=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(score.view(torch.int64), want["score"].view(torch.int64)) and bool((part == 7.0).all()) and bool((skipped == 7).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(part.view(torch.int64), want["part"].view(torch.int64)) and torch.equal(skipped, want["skipped"])
    assert call(S_=0, A_=0) == 0                                                # an empty block launches nothing
    none = boreholes.score(ens, t["rows"], t["nu"], dict(att, att_ptr=np.zeros(S + 1, dtype=np.int32), att_sounding=np.zeros(0, np.int32), att_bore=np.zeros(0, np.int32),
                                                        att_var=np.zeros(0), att_shift=np.zeros(0)), logs, classes=CLASSES)
    assert none["part"].shape == (0, n) and bool((none["score"].view(torch.int64) == 0).all())


def _planted():
    k, edges, sigma, x, y, ptr, truth = planted_lines()
    return _to_device(k, edges, sigma), edges, x, y, ptr, truth


def _same(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for name in a:
        va, vb = a[name], b[name]
        assert va.dtype == vb.dtype and va.shape == vb.shape, (what, name)
        assert np.array_equal(va.view(np.int64) if va.dtype == np.float64 else va, vb.view(np.int64) if vb.dtype == np.float64 else vb), (what, name)


BOREHOLE_KEYS = ("borehole_score", "borehole_sounding", "borehole_index", "borehole_distance", "borehole_skipped", "borehole_log_predictive")


def test_the_keyword_is_the_score_handed_on_bit_for_bit():
    ens, _, x, y, ptr, truth = _planted()
    S, n = ens.k.shape
    depth_edges = np.arange(0.0, Z1_LINES + 1.0, 5.0)
    logs = boreholes.Logs([75.0, 30.0], [100.0, 40.0], None, [0, 50, 51], np.concatenate([planted_log("induction", truth).top, [3.0]]),
                          np.concatenate([planted_log("induction", truth).bottom, [33.0]]), np.concatenate([planted_log("induction", truth).value, [np.nan]]),
                          np.concatenate([planted_log("induction", truth).sd, [np.nan]]), np.concatenate([np.full(50, -1), [1]]))
    opt = dict(logs=logs, max_distance=70.0, classes=LITH_CLASSES)            # the second log reaches the first and the middle line
    kw = dict(ptr=ptr, max_models=n, draws=8, seed=5, products=dict(depth_edges=depth_edges), bodies=dict(depth_edges=depth_edges, lo=-1.0, hi=0.0))
    with_logs = _numpy(sections.sections(ens, x, y, Z1_LINES, boreholes=opt, **kw))
    assert set(BOREHOLE_KEYS) <= set(with_logs) and with_logs["borehole_sounding"].tolist() == [1, BORE_ROW - 2, BORE_ROW]
    assert with_logs["borehole_index"].tolist() == [1, 1, 0] and with_logs["borehole_distance"][2] == 0.0 and with_logs["borehole_skipped"].tolist() == [0, 0, 0]
    handed = _numpy(sections.sections(ens, x, y, Z1_LINES, score=torch.as_tensor(with_logs["borehole_score"]).to(_dev()), **kw))
    _same({name: v for name, v in with_logs.items() if name not in BOREHOLE_KEYS}, handed, "sections")
    extra = torch.as_tensor(np.random.default_rng(3).normal(size=(S, n))).to(_dev())
    both = _numpy(sections.sections(ens, x, y, Z1_LINES, score=extra, boreholes=opt, **kw))      # added to the caller's score
    summed = _numpy(sections.sections(ens, x, y, Z1_LINES, score=extra + torch.as_tensor(with_logs["borehole_score"]).to(_dev()), **kw))
    _same({name: v for name, v in both.items() if name not in BOREHOLE_KEYS}, summed, "sections with a score")
    plain, none = _numpy(sections.sections(ens, x, y, Z1_LINES, **kw)), _numpy(sections.sections(ens, x, y, Z1_LINES, boreholes=None, **kw))
    _same(plain, none, "sections, boreholes=None")
    assert not np.array_equal(plain["weight"], with_logs["weight"])
    no_marginals = sections.sections(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, marginals=False, boreholes=opt)
    assert "borehole_log_predictive" not in no_marginals and "borehole_score" in no_marginals

    skw = dict(ptr=ptr, max_models=n, max_distance=150.0, sweeps=12, draws=8, seed=5, draw_sweeps=3, products=dict(depth_edges=depth_edges),
               bodies=dict(depth_edges=depth_edges, lo=-1.0, hi=0.0))
    across = _numpy(sections.spatial(ens, x, y, Z1_LINES, boreholes=opt, **skw))
    assert set(BOREHOLE_KEYS) <= set(across) and np.array_equal(_bits(across["borehole_score"]), _bits(with_logs["borehole_score"]))
    handed = _numpy(sections.spatial(ens, x, y, Z1_LINES, score=torch.as_tensor(across["borehole_score"]).to(_dev()), **skw))
    _same({name: v for name, v in across.items() if name not in BOREHOLE_KEYS}, handed, "spatial")
    _same(_numpy(sections.spatial(ens, x, y, Z1_LINES, **skw)), _numpy(sections.spatial(ens, x, y, Z1_LINES, boreholes=None, **skw)), "spatial, boreholes=None")


@pytest.mark.parametrize("kind", ["induction", "lithology"])
def test_one_log_decides_the_planted_line_on_the_device(kind):
    ens, edges, x, y, ptr, truth = _planted()
    S, n = ens.k.shape
    middle = np.arange(S_LINES, 2 * S_LINES)
    logs = planted_log(kind, truth)
    opt = dict(logs=logs, max_distance=1.0, classes=LITH_CLASSES if kind == "lithology" else None)
    alone = sections.sections(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, draws=64, seed=2)
    cond = sections.sections(ens, x, y, Z1_LINES, ptr=ptr, max_models=n, draws=64, seed=2, boreholes=opt)
    a, c = _numpy(alone), _numpy(cond)
    assert np.all(a["state"][middle] < 10) and np.all(a["weight"][middle, :10].sum(axis=1) > 0.625)
    assert np.all(c["state"][middle] >= 10) and np.all(c["weight"][middle, :10].sum(axis=1) < 1e-3)
    assert np.all(np.abs(edges[middle, c["state"][middle], 0] - truth[middle]) <= 4.0)
    assert np.all(c["draw_state"][:, middle] >= 10) and np.any(a["draw_state"][:, middle] < 10)      # all 64 draws in the true family
    outer = np.concatenate([np.arange(S_LINES), np.arange(2 * S_LINES, S)])
    assert np.array_equal(a["state"][outer], c["state"][outer]) and np.array_equal(_bits(a["weight"][outer]), _bits(c["weight"][outer]))
    assert c["borehole_sounding"].tolist() == [BORE_ROW] and c["borehole_skipped"].tolist() == [0]
    sc = c["borehole_score"]
    assert np.all(sc[np.arange(S) != BORE_ROW] == 0.0) and sc[BORE_ROW, :10].max() < sc[BORE_ROW, 10:].min() - 50.0
    # the blind test: the section that has not seen the log predicts it worse than the one that has
    att = boreholes.attach(x, y, logs, ptr, a["n_used"], max_distance=1.0)
    part = boreholes.score(ens, alone["rows"], alone["n_used"], att, logs, classes=opt["classes"])["part"]
    blind = boreholes.log_predictive(part, alone["weight"], alone["n_used"], att).cpu().numpy()
    w = a["weight"][BORE_ROW].astype(np.longdouble)
    want = float(np.log((w * np.exp(part.cpu().numpy()[0].astype(np.longdouble))).sum()))
    print("%s: log predictive blind %.3f, conditioned %.3f" % (kind, blind[0], c["borehole_log_predictive"][0]))
    assert abs(blind[0] - want) <= 1e-12 * abs(want) and blind[0] < c["borehole_log_predictive"][0] <= 0.0


def test_from_survey_and_the_command_line(tmp_path):
    k, edges, sigma, x, y, ptr, truth = planted_lines()
    survey = dict(ensemble_k=k, ensemble_edges=edges, ensemble_sigma=sigma, line=np.repeat([10, 20, 30], S_LINES), x=x, y=y, fiducial=np.arange(k.shape[0]))
    logs = planted_log("lithology", truth)
    table = boreholes.save(logs, str(tmp_path / "logs.csv"))
    opt = dict(logs=logs, max_distance=1.0, classes=LITH_CLASSES, class_floor=1e-5)
    direct = _numpy(sections.from_survey(survey, Z1_LINES, max_models=16, draws=4, boreholes=opt))
    by_path = _numpy(sections.from_survey(survey, Z1_LINES, max_models=16, draws=4, boreholes=dict(opt, logs=table)))
    _same({n: np.asarray(v) for n, v in direct.items()}, {n: np.asarray(v) for n, v in by_path.items()}, "logs as a path")
    assert np.all(direct["state"][S_LINES:2 * S_LINES] >= 10)
    # with elevations and finite collars the survey's surface is the default: a collar 5 m above the ground skips nothing but shifts the log
    raised = boreholes.Logs(logs.x, logs.y, [105.0], logs.ptr, logs.top, logs.bottom, logs.value, logs.sd, logs.cls)
    shifted = _numpy(sections.from_survey(dict(survey, elevation=np.full(k.shape[0], 100.0)), Z1_LINES, max_models=16, boreholes=dict(opt, logs=raised)))
    assert shifted["borehole_skipped"].tolist() == [2] and not np.array_equal(shifted["borehole_score"], direct["borehole_score"])
    path = str(tmp_path / "survey.npz")
    np.savez(path, **survey)
    args = ["--boreholes", table, "--borehole-distance", "1", "--class-means", "-2", "-0.5", "-1.5", "--class-scales", "0.2", "0.2", "0.2", "--class-floor", "1e-5"]
    written = sections.main([path, "--depth", "120", "--max-models", "16", "--draws", "4"] + args)
    f = sections.load(written)
    assert set(BOREHOLE_KEYS) <= set(f) and set(f) == set(direct)
    assert all(np.array_equal(f[name], direct[name], equal_nan=True) for name in direct)
    written = sections.main([path, "--depth", "120", "--max-models", "16", "--spatial", "150", "--spatial-draws", "4", "--depth-axis", "24", "5", "--bodies", "-1", "0"] + args)
    f = sections.load(written)
    assert written.endswith(".spatial.npz") and set(BOREHOLE_KEYS) <= set(f) and "body_count" in f and np.all(f["state"][S_LINES:2 * S_LINES] >= 10)
    assert np.array_equal(f["borehole_score"], direct["borehole_score"])
