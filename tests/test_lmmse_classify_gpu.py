"""``aft_lmmse_classify_f32``, ``hip_ops.LmmseClassifyPlan``, ``lmmse.ConditionEstimator`` and ``LmmseEstimator(conditions="estimated")``
on the HIP device: the kernel's scores against the float64 twin's within a DERIVED bound, its choice against its own scores exactly and
against the twin's wherever the bound separates the best candidate from the rest, the bit identities (NULL scores, batch and position,
pinned pilots, the checked build, the blind module against ``LmmseSeqPlan`` fed the plan's own outputs), no unwritten output, no
synchronisation, the entry point's refusals.

The bound (``score_bound``), in the manner of ``test_lmmse_gpu.derived_bound``: u = 2^-24, gamma(n) = n u / (1 - n u), the device reads
float32 roundings of the table entries and the pilots exactly, every product stage of k_lmmse_classify.hip is a chain of fused
multiply-adds.  Per member a, element (k, l) and candidate (s, d, e), with |.| for element-wise moduli:

* Y1 = U_f^H P:     e1 = ((1 + u)(1 + sqrt(2) gamma(2 Ps)) - 1) |U_f^H||P|,                       m1 = |U_f^H||P| + e1
* Z  = Y1 U_t:      e2 = e1 |U_t| + ((1 + u)(1 + gamma(w Pt)) - 1) m1 |U_t|     (the sibling kernel's two stages, the same chains)
* |Z|^2:            ||Zd|^2 - |Z|^2| <= e2 (2 |Z| + e2) with the definition's own |Z|; the kernel forms re re + (im im + acc) with
                    two fused multiply-adds per member, all terms non-negative: a factor within gamma(2 m) on the sum over the m
                    members.     dE = sum_a e2 (2 |Z| + e2) + gamma(2 m) sum_a (|Z| + e2)^2
* V = lf lt + s2:   three rounded non-negative inputs, one fused multiply-add: within ex = (1 + u)^3 - 1; the division within 2.5 ulp
                    (test_lmmse_gpu's model):  rD = (1 + ex / (1 - ex))(1 + 5 u) - 1,       dt = rD E / V + (1 + rD) dE / V
* Q = sum_kl t:     non-negative terms added in a tree whose longest chain is D = ceil(Ps w Pt / 256) (a thread's own elements) + 6
                    (the shuffles 32 .. 1) + 3 (at most four waves), read off the kernel's step 4:
                    dQ = sum dt + gamma(D) (Q + sum dt)
* score = -fma(m, logdet, Q): the table entry is a float32 rounding (u m |logdet|), the fused multiply-add rounds once:
                    bound = u m |logdet| + dQ + u (|score| + u m |logdet| + dQ)
No measured constant enters.  The bound is evaluated on absolute values in the two product stages, so it sits well above what is
observed (printed per case); a case of the first three whose ambiguous share passes 10 % would mean it is too loose."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, _lib
from adafortitran_amd.chansim import ChannelSimConfig, simulate_frames_host
from adafortitran_amd.hip_ops import LmmseClassifyPlan, LmmsePlan, LmmseSeqPlan
from adafortitran_amd.lmmse import ConditionEstimator, LmmseEstimator, LmmseTables, lmmse_classify_host
from test_chansim_gpu import _bits, _no_sync, _poison, _same_bits
from test_lmmse_gpu import U, _dev, _gamma

pytestmark = pytest.mark.gpu
DEV = "cuda"


def score_bound(tb: LmmseTables, pilots: np.ndarray, pool: bool) -> np.ndarray:
    """Bound on |device score - twin's score| per (unit, candidate), [units, n_snr n_ds n_dop]; module docstring.  0 where nothing is
    computed (w = 0)."""
    cfg = tb.cfg
    Ps, Pt = cfg.pilot
    K = cfg.slots if tb.multi_slot else 1
    G = cfg.group if (tb.multi_slot or pool) else 1
    m = G if pool else 1
    n_snr, n_ds, n_dop = (len(tb.values[k]) for k in ("snr_db", "delay_spread_ns", "doppler_hz"))
    units = len(pilots) // m
    head = np.arange(units) * m
    ws = tb.slot_window(head // G % K)
    p_all = np.asarray(pilots).astype(np.complex128)
    r2 = np.sqrt(2.0)
    cc = (1 + U) * (1 + r2 * _gamma(2 * Ps)) - 1
    ex = (1 + U) ** 3 - 1
    r_d = (1 + ex / (1 - ex)) * (1 + 5 * U) - 1
    out = np.zeros((units, n_snr * n_ds * n_dop))
    for w in np.unique(ws[ws > 0]):
        w = int(w)
        sel = np.nonzero(ws == w)[0]
        frames = head[sel][:, None] + np.arange(m)[None, :]
        src = frames[:, :, None] - (tb.horizon + w - 1 - np.arange(w))[None, None, :] * G
        p = p_all[src].transpose(0, 1, 3, 2, 4).reshape(len(sel), m, Ps, w * Pt)
        cr = (1 + U) * (1 + _gamma(w * Pt)) - 1
        depth = -(-(Ps * w * Pt) // 256) + 6 + 3
        for d in range(n_ds):
            ufh = tb.u_f[d].conj().T
            a1 = np.einsum("ki,umij->umkj", np.abs(ufh), np.abs(p))
            e1 = cc * a1
            y1 = np.einsum("ki,umij->umkj", ufh, p)
            for e in range(n_dop):
                lam_t, u_t, _ = tb.time(e, w)
                z = np.abs(np.einsum("umkj,jl->umkl", y1, u_t))
                e2 = np.einsum("umkj,jl->umkl", e1, np.abs(u_t)) + cr * np.einsum("umkj,jl->umkl", a1 + e1, np.abs(u_t))
                energy = (z ** 2).sum(axis=1)
                d_e = (e2 * (2 * z + e2)).sum(axis=1) + _gamma(2 * m) * ((z + e2) ** 2).sum(axis=1)
                v = (tb.lam_f[d][:, None] * lam_t[None, :])[None] + tb.sigma2[:, None, None]              # [s, k, l]
                q = np.einsum("ukl,skl->us", energy, 1.0 / v)
                d_t = r_d * q + (1 + r_d) * np.einsum("ukl,skl->us", d_e, 1.0 / v)
                d_q = d_t + _gamma(depth) * (q + d_t)
                ld = m * np.abs(tb.logdet(d, e, w))[None, :]
                score = np.abs(m * tb.logdet(d, e, w)[None, :] + q)
                bound = U * ld + d_q + U * (score + U * ld + d_q)
                for s in range(n_snr):
                    out[sel, (s * n_ds + d) * n_dop + e] = bound[:, s]
    return out


def _argmax(scores: np.ndarray, lowest: int = 0) -> np.ndarray:
    """The tie rule on a score array: the lowest index of the highest score, a NaN never wins, all -inf / NaN -> ``lowest``."""
    ranked = np.where(np.isnan(scores), -np.inf, scores)
    return np.where(np.isneginf(ranked.max(axis=1)), lowest, ranked.argmax(axis=1))


def _reach(want: np.ndarray, bound: np.ndarray, best: np.ndarray) -> np.ndarray:
    """[units, candidates]: the candidates whose interval ``[score - bound, score + bound]`` reaches the best one's, the best included.
    Where both bounds are 0 the scores are exact (nothing was computed) and the tie rule has decided: no other candidate reaches."""
    rows = np.arange(len(want))
    lo, b0 = (want[rows, best] - bound[rows, best])[:, None], bound[rows, best][:, None]
    reach = (want + bound >= lo) & (bound + b0 > 0)
    reach[rows, best] = True
    return reach


_SMALL = dict(ofdm=(24, 6), pilot=(5, 2), slots=4, slot_symbols=6)
# name: (config, W, h, frames, the ambiguous share is capped)
CASES = {
    "default_single_slot": (ChannelSimConfig(), 1, 0, 256, True),
    "default_slots8_w4": (ChannelSimConfig(slots=8), 4, 0, 32 * 8, True),
    "odd_group_zero_slot_every_w": (ChannelSimConfig(antennas=(2, 1), **_SMALL), 3, 1, 32 * 4 * 2, True),   # odd Ps, a group, w = 0 .. 3
    "default_w8_narrow_tiles": (ChannelSimConfig(slots=9), 8, 0, 9, False),                                # W Pt = 16: 24 KB of LDS
    "default_w9_wide_tiles": (ChannelSimConfig(slots=9), 9, 0, 9, False),                                  # W Pt = 18: 40 KB
    "lds_bound_128x40": (ChannelSimConfig(ofdm=(128, 40), pilot=(64, 16), slots=2), 2, 0, 4, False),       # Ps w Pt = 2048: chunks of one
    "degenerate_1x1_group_16": (ChannelSimConfig(ofdm=(1, 1), pilot=(1, 1), antennas=(4, 4), slots=3), 1, 2, 2 * 3 * 16, False),
}
_cache = {}


def _case(name):
    """(cfg, tables, plan, pilots complex64, twin idx, twin scores, bound), made once per case and left unchanged."""
    if name not in _cache:
        cfg, W, h, frames, _ = CASES[name]
        tb = LmmseTables(cfg, W, h)
        _, pilots, _ = simulate_frames_host(cfg, 11, np.arange(frames))
        pilots = pilots.astype(np.complex64)
        idx, _, scores = lmmse_classify_host(tb, pilots, return_scores=True)
        bound = score_bound(tb, pilots, True)
        for a in (pilots, idx, scores, bound):
            a.setflags(write=False)
        _cache[name] = (cfg, tb, LmmseClassifyPlan(tb, DEV), pilots, idx, scores, bound)
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_scores_and_choice_against_the_float64_twin(name):
    cfg, tb, plan, pilots, want_idx, want, bound = _case(name)
    capped = CASES[name][4]
    b, units, ncand = len(pilots), len(want), want.shape[1]
    m = b // units
    assert plan.logdet.numel() == _lib.load().aft_lmmse_classify_table_floats(ctypes.byref(plan.plan), tb.window) == 49 * tb.window * 7
    shapes = [((b, 3), torch.int32), ((b,), torch.float32), ((b,), torch.float32), ((b,), torch.float32), ((units, ncand), torch.float32)]
    poison = [((b, 3), torch.float32)] + shapes[1:]               # idx as floats of its size: NaN bits are no index below 7
    _poison(poison)                                               # an element the kernel leaves unwritten would come back NaN
    idx, snr, ds, dop, sc = plan(_dev(pilots), scores=True)
    assert [(tuple(t.shape), t.dtype) for t in (idx, snr, ds, dop, sc)] == shapes and all(t.is_cuda for t in (idx, snr, ds, dop, sc))
    got, gi = sc.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    assert np.isfinite(got).all() and (gi >= 0).all() and (gi < 7).all()
    for k, (vals, col) in enumerate(zip((tb.values["snr_db"], tb.values["delay_spread_ns"], tb.values["doppler_hz"]), (snr, ds, dop))):
        assert np.array_equal(col.cpu().numpy(), vals[gi[:, k]].astype(np.float32))              # the table values of the choice
    assert np.array_equal(gi, np.repeat(gi[::m], m, axis=0))                                       # a group's members share it
    err = np.abs(got - want)
    live = bound > 0
    print(f"{name}: max|score - twin| {err.max():.3e} (|score| up to {np.abs(want).max():.3e})   largest err / bound "
          f"{float((err[live] / bound[live]).max()) if live.any() else 0.0:.3f}   bound up to {bound.max():.3e}")
    assert (err <= bound).all()
    assert not _bits(sc[torch.from_numpy(~live.any(axis=1)).to(DEV)]).any()                        # nothing to look at: +0.0 scores
    # the choice is the argmax of the device's OWN scores under the tie rule, exactly; and the same bits without the scores
    flat = (gi[::m, 0] * 7 + gi[::m, 1]) * 7 + gi[::m, 2]
    assert np.array_equal(flat, _argmax(got))
    _poison(poison[:4])
    _same_bits(plan(_dev(pilots)), [idx, snr, ds, dop])
    # ... and the twin's wherever no other candidate's interval reaches the best one's; among the overlapping ones otherwise
    best = (want_idx[::m, 0] * 7 + want_idx[::m, 1]) * 7 + want_idx[::m, 2]
    rows = np.arange(units)
    reach = _reach(want, bound, best)
    ambiguous = reach.sum(axis=1) > 1
    print(f"{name}: {int(ambiguous.sum())} of {units} units ambiguous ({ambiguous.mean():.1%}); device = twin on "
          f"{float((flat == best).mean()):.1%} of all units")
    assert np.array_equal(flat[~ambiguous], best[~ambiguous])
    assert reach[rows, flat].all()
    if capped:
        assert ambiguous.mean() <= 0.10


def test_both_lds_variants_give_the_same_bits():
    """Slots 0 .. 7 of a 9-slot sequence have the same windows and tables under W = 8 (narrow tiles) and W = 9 (wide tiles)."""
    _, tb8, narrow, pilots, *_ = _case("default_w8_narrow_tiles")
    _, tb9, wide, pilots9, *_ = _case("default_w9_wide_tiles")
    assert np.array_equal(pilots, pilots9)
    a, b = narrow(_dev(pilots), scores=True), wide(_dev(pilots), scores=True)
    _same_bits([t[:8] for t in a], [t[:8] for t in b])


def test_bits_do_not_depend_on_batch_or_position():
    for name in ("default_slots8_w4", "odd_group_zero_slot_every_w"):
        cfg, tb, plan, pilots, *_ = _case(name)
        unit = cfg.sequence()
        full = plan(_dev(pilots), scores=True)
        alone = plan(_dev(pilots[:unit]), scores=True)
        per = len(full[4]) // (len(pilots) // unit)                                               # score rows per sequence
        _same_bits(alone, [t[:unit] for t in full[:4]] + [full[4][:per]])
        _, many, _ = simulate_frames_host(cfg, 13, np.arange(5 * unit))
        many = many.astype(np.complex64)
        for pos in (1, 4):
            many[pos * unit:(pos + 1) * unit] = pilots[:unit]
        batch = plan(_dev(many), scores=True)
        for pos in (1, 4):
            _same_bits([t[pos * unit:(pos + 1) * unit] for t in batch[:4]] + [batch[4][pos * per:(pos + 1) * per]], alone)
        # a window cut out of the longer sequence: slot k of K against the last slot of the W slots that end there
        W, K, G = tb.window, cfg.slots, cfg.group
        if tb.horizon == 0:
            short = LmmseClassifyPlan(LmmseTables(dataclasses.replace(cfg, slots=W), W, 0), DEV)
            for k in range(W - 1, K):
                cut = short(_dev(pilots[(k - W + 1) * G:(k + 1) * G]), scores=True)
                _same_bits([t[-G:] for t in cut[:4]] + [cut[4][-1:]], [t[k * G:(k + 1) * G] for t in full[:4]] + [full[4][k:k + 1]])


def test_pinned_host_pilots_give_the_same_bits():
    _, _, plan, pilots, *_ = _case("odd_group_zero_slot_every_w")
    _same_bits(plan(torch.from_numpy(np.array(pilots)).pin_memory(), scores=True), plan(_dev(pilots), scores=True))
    with pytest.raises(ValueError, match="pinned host memory"):
        plan(torch.from_numpy(np.array(pilots)))
    with pytest.raises(ValueError, match="HIP device"):
        LmmseClassifyPlan(plan.tables, "cpu")
    with pytest.raises(ValueError, match="log-determinant table"):
        LmmseClassifyPlan(plan.tables, DEV, logdet=plan.logdet[:-1])


def test_pins_and_frames_that_decide_alone():
    """``assume`` with one, two and three pins and ``pool=False`` on the grouped case: the twin's rules (excluded candidates read -inf,
    all three pinned computes nothing) and its scores within the bound."""
    cfg, tb, _, pilots, _, _, _ = _case("odd_group_zero_slot_every_w")
    for assume, pool in ((dict(snr_db=10), True), (dict(snr_db=10, doppler_hz=1400), True),
                         (dict(snr_db=10, delay_spread_ns=350, doppler_hz=1400), True), (None, False)):
        plan = LmmseClassifyPlan(tb, DEV, assume=assume, pool=pool)
        want_idx, want_val, want = lmmse_classify_host(tb, pilots, assume, pool, return_scores=True)
        idx, snr, ds, dop, sc = plan(_dev(pilots), scores=True)
        got, gi = sc.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
        out = np.isneginf(want)
        assert np.array_equal(np.isneginf(got), out) and not np.isnan(got).any()
        bound = score_bound(tb, pilots, pool)
        assert (np.abs(got[~out] - want[~out]) <= bound[~out]).all()
        m = len(pilots) // len(want)
        lowest = int(np.flatnonzero(~out[0])[0])
        flat = (gi[::m, 0] * 7 + gi[::m, 1]) * 7 + gi[::m, 2]
        assert np.array_equal(flat, _argmax(got, lowest))
        for k, f in enumerate(tb.fixed(assume)):
            if f >= 0:
                assert (gi[:, k] == f).all()
        if assume is not None and len(assume) == 3:
            assert np.array_equal(gi, want_idx) and not got[~out].any()                            # nothing computed: +0, the pins
        _same_bits(plan(_dev(pilots)), [idx, snr, ds, dop])
        rows = np.arange(len(want))
        best = (want_idx[::m, 0] * 7 + want_idx[::m, 1]) * 7 + want_idx[::m, 2]
        reach = _reach(want, bound, best)
        assert reach[rows, flat].all()


def test_nan_pilots_choose_index_zero():
    cfg, tb, plan, pilots, *_ = _case("default_slots8_w4")
    bad = np.array(pilots[:8])
    bad[3, 0, 0] = np.nan                                          # slot 3 of the sequence: every window that holds it is all NaN
    idx, snr, ds, dop, sc = plan(_dev(bad), scores=True)
    want_idx, _ = lmmse_classify_host(tb, bad)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and not want_idx[3:7].any()
    assert torch.isnan(sc[3:7]).all() and torch.isfinite(sc[:3]).all() and torch.isfinite(sc[7]).all()


def test_checked_build_gives_the_same_bits():
    path = os.path.join(os.path.dirname(_lib.lib_path()), "libaft_hip_check.so")
    if not os.path.exists(path) or not hasattr(ctypes.CDLL(path), "aft_lmmse_classify_f32"):     # missing, or left by an earlier tree
        from adafortitran_amd import build
        build.build_checked()
    lib = _lib.load_path(path)
    assert lib.aft_version() == _abi.AFT_ABI_VERSION and hasattr(lib, "aft_lmmse_classify_f32")
    for name in CASES:
        _, _, plan, pilots, *_ = _case(name)
        _same_bits(plan(_dev(pilots), scores=True, lib=lib), plan(_dev(pilots), scores=True))


def test_blind_module_is_classify_then_estimate_without_a_synchronisation():
    """``LmmseEstimator(conditions="estimated")`` equals ``LmmseSeqPlan`` fed the classify plan's own outputs, bit for bit, from device
    and from CPU pilots (the pinned ring), with no synchronisation; ``ConditionEstimator`` is the plan."""
    for cfg, W, h in ((ChannelSimConfig(slots=4, antennas=(1, 2)), 4, 0), (ChannelSimConfig(), 1, 0)):
        unit = cfg.sequence() * (1 if W > 1 else 4)
        tb = LmmseTables(cfg, W, h)
        _, pilots, meta = simulate_frames_host(cfg, 11, np.arange(3 * unit))
        pilots = torch.from_numpy(pilots.astype(np.complex64))
        model = LmmseEstimator(cfg, window=W, horizon=h, conditions="estimated").to(DEV).eval()
        chooser = ConditionEstimator(cfg, W, h).to(DEV)
        cplan = LmmseClassifyPlan(tb, DEV)
        eplan = (LmmseSeqPlan if tb.multi_slot else LmmsePlan)(tb, DEV)
        batches = [pilots[i * unit:(i + 1) * unit] for i in range(3)]
        first = model(batches[0].to(DEV), None)                      # builds the plans: outside the guard
        model(batches[0], None)                                      # ... and pins the ring
        chooser(batches[0])
        torch.cuda.synchronize()
        probe = torch.ones((), device=DEV)
        with _no_sync():
            with pytest.raises(RuntimeError):
                probe.item()                                         # the mode is honoured: what follows is not vacuous
            resident = [model(p, None) for p in batches]
            conds = [chooser(p) for p in batches]
        dev_batches = [p.to(DEV) for p in batches]
        for p, est, cond in zip(dev_batches, resident, conds):
            idx, snr, ds, dop = cplan(p)
            _same_bits(cond, [snr, ds, dop])
            _same_bits([est], [eplan(p, snr, ds, dop)])
            _same_bits([model(p, None)], [est])                      # device-resident pilots: the same bits as through the ring
        _same_bits([first], [resident[0]])
        bogus = (None, torch.full((unit, 1), float("nan")), torch.zeros(unit, 1), torch.zeros(unit, 1), None, None)
        _same_bits([model(batches[0], bogus)], [first])              # the meta's conditions are ignored
    grouped = LmmseEstimator(ChannelSimConfig(antennas=(1, 2)), conditions="estimated").to(DEV)
    with pytest.raises(ValueError, match="not whole groups"):
        grouped(pilots[:3].to(DEV), None)


def test_estimated_conditions_around_adafortitran_is_a_meta_substitution():
    """``EstimatedConditions(AdaFortiTranEstimator)`` on the device: the wrapped model's output equals the model called by hand with the
    classify plan's own outputs in the six-tuple, bit for bit, with or without a meta, and ``get_test_stats`` measures the wrapper."""
    import adafortitran_amd as A
    from adafortitran_amd import ingest
    from adafortitran_amd.chansim import make_pack
    from adafortitran_amd.evaluation import get_test_stats
    from adafortitran_amd.lmmse import EstimatedConditions
    cfg = ChannelSimConfig()
    sc = A.SystemConfig(ofdm=dict(num_scs=120, num_symbols=14), pilot=dict(num_scs=12, num_symbols=2))
    mc = A.ModelConfig(model_type="adafortitran", patch_size=(3, 2), num_layers=2, model_dim=128, num_head=4, activation="gelu",
                       max_seq_len=512, pos_encoding_type="learnable", device=DEV, dropout=0.0,
                       channel_adaptivity_hidden_sizes=[7, 42, 560], adaptive_token_length=6)
    torch.manual_seed(3)
    model = A.AdaFortiTranEstimator(sc, mc).eval()
    wrapped = EstimatedConditions(model, cfg).to(DEV).eval()
    _, pilots, meta = simulate_frames_host(cfg, 11, np.arange(16))
    pil = _dev(pilots.astype(np.complex64))
    given = (torch.arange(16), *(torch.from_numpy(np.ascontiguousarray(meta[:, k:k + 1])) for k in range(3)), 8, ["a"])
    _, snr, ds, dop = LmmseClassifyPlan(LmmseTables(cfg), DEV)(pil)
    by_hand = (given[0], snr.reshape(-1, 1), ds.reshape(-1, 1), dop.reshape(-1, 1), 8, ["a"])
    with torch.no_grad():
        want = model(pil, by_hand)
        _same_bits([wrapped(pil, given)], [want])
        _same_bits([wrapped(pil)], [want])
        assert not torch.equal(_bits(model(pil, given)), _bits(want))                     # the tokens matter: the genie's differ
    assert all(torch.equal(a, b) for a, b in zip(wrapped.substitute(pil, given)[1:4], by_hand[1:4]))
    packs = {snr_db: make_pack(cfg, 32, seed=50 + snr_db, snr_db=snr_db) for snr_db in (0, 20)}
    loaders = [(f"SNR_{k}", ingest.ResidentLoader(p, cfg.pilot, 16, device=DEV, shuffle=False)) for k, p in packs.items()]
    stats = get_test_stats(wrapped, loaders)
    assert list(stats) == [0, 20] and all(np.isfinite(v) for v in stats.values())


def test_every_refusal_of_the_entry_point_launches_nothing():
    cfg, tb, plan, pilots, *_ = _case("default_slots8_w4")
    lib, b = _lib.load(), len(pilots)
    idx = torch.full((b, 3), -7, dtype=torch.int32, device=DEV)
    outs = [torch.full((b,), float("nan"), device=DEV) for _ in range(3)]
    sc = torch.full((b, 343), float("nan"), device=DEV)
    pil = _dev(pilots)
    good = dict(group=1, slots=8, window=4, horizon=0, pool=1, tables=plan.image.data_ptr(), logdet=plan.logdet.data_ptr(),
                pilots=pil.data_ptr(), idx=idx.data_ptr(), snr=outs[0].data_ptr(), ds=outs[1].data_ptr(), dop=outs[2].data_ptr(),
                scores=sc.data_ptr(), batch=b)

    def call(p=None, **kw):
        a = dict(good, **kw)
        return lib.aft_lmmse_classify_f32(ctypes.byref(p if p is not None else tb.to_struct()), a["group"], a["slots"], a["window"],
                                          a["horizon"], a["pool"], a["tables"], a["logdet"], a["pilots"], a["idx"], a["snr"], a["ds"],
                                          a["dop"], a["scores"], a["batch"], None)

    def refused(code, word, p=None, **kw):
        rc = call(p, **kw)
        assert rc == code and word in lib.aft_last_error().decode(), (rc, lib.aft_last_error())

    E, SH = _abi.AFT_ERR_ARG, _abi.AFT_ERR_SHAPE
    rc = lib.aft_lmmse_classify_f32(None, 1, 8, 4, 0, 1, *(good[k] for k in ("tables", "logdet", "pilots", "idx", "snr", "ds", "dop", "scores")), b, None)
    assert rc == E and "NULL" in lib.aft_last_error().decode()
    for k in ("tables", "logdet", "pilots", "idx", "snr", "ds", "dop"):
        refused(E, "NULL pointer", **{k: None})
    for k in ("tables", "pilots"):
        refused(E, "8-byte", **{k: good[k] + 4})
    for k in ("logdet", "idx", "snr", "ds", "dop", "scores"):
        refused(E, "4-byte", **{k: good[k] + 2})
    for batch in (0, -3):
        refused(E, "batch must be at least 1", batch=batch)
    for batch in (b - 1, 12):
        refused(E, "is not a multiple of slots * group = 8 * 1", batch=batch)
    refused(E, "is not a multiple of slots * group = 8 * 3", group=3, batch=b)
    for pool in (-1, 2):
        refused(E, "pool must be 0", pool=pool)
    for field, value, word in (("num_scs", 0, "num_scs = 0"), ("pilot_symbols", 17, "pilot_symbols = 17 is outside 1..16"),
                               ("n_dop", 17, "n_dop = 17"), ("fixed_snr", 7, "fixed_snr = 7 is outside -1..6"),
                               ("num_symbols", 1, "larger than the ofdm grid")):
        p = tb.to_struct()
        setattr(p, field, value)
        refused(SH, word, p=p)
        assert lib.aft_lmmse_classify_table_floats(ctypes.byref(p), 4) == 0
    for kw, word in ((dict(group=0), "group = 0 is outside 1..16"), (dict(group=17), "group = 17 is outside 1..16"),
                     (dict(slots=0), "slots = 0 is outside 1..4096"), (dict(window=0), "window = 0 is outside 1..8"),
                     (dict(window=9), "window = 9 is outside 1..8"), (dict(slots=32, window=17), "window * pilot_symbols = 34 is outside 1..32"),
                     (dict(horizon=-1), "horizon = -1 is outside 0..7"), (dict(horizon=8), "horizon = 8 is outside 0..7")):
        refused(SH, "lmmse classify: " + word, **kw)                 # the refusal names the entry point that was called
    assert lib.aft_lmmse_classify_table_floats(None, 4) == 0 and lib.aft_lmmse_classify_table_floats(ctypes.byref(tb.to_struct()), 0) == 0
    torch.cuda.synchronize()
    assert (idx == -7).all() and all(torch.isnan(t).all() for t in outs) and torch.isnan(sc).all()      # nothing was launched
    assert call(scores=None) == _abi.AFT_OK
    torch.cuda.synchronize()
    assert (idx >= 0).all() and all(torch.isfinite(t).all() for t in outs) and torch.isnan(sc).all()
    assert call() == _abi.AFT_OK
    torch.cuda.synchronize()
    assert torch.isfinite(sc).all()                                                                        # ... and the good call writes it all
