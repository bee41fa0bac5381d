"""``linksim``'s codeword-cancellation link on the CPU: ``link_cancel_host`` against ``link_sic_host(genie=True)`` exactly wherever that
detects the stream second, against a brute force over all ``2^m`` symbols of the cancelled sample, against the diversity link with an
unheard other stream, the exact extreme and the all-zero streams; ``cwsic_redetect``'s truth table; ``link_cwsic_host`` against its
parts; ``LdpcBlockErrorAccumulator(detector="cwsic")`` on a CPU device against the ``detector="mmse"`` accumulator and against a
batch-by-batch recomputation from the definition, on one rank and on two (gloo); every refusal; the pinned constants; and the physical
conditions on the inputs tests/test_linkcwsic_gpu.py runs the device on (``physical_inputs``, made once and shared)."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch

from adafortitran_amd import _abi, linksim
from adafortitran_amd.chansim import ChannelSimConfig, SynthLoader, frame_keys, ls_interpolate, make_pack
from adafortitran_amd.linksim import (ALL_DETECTORS, BITS_PER_SYMBOL, DETECTORS, LINK2_DETECTORS, BlockErrorAccumulator, CodeConfig,
                                      HarqAccumulator, HarqConfig, LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator, LinkConfig,
                                      RateAccumulator, cwsic_final, cwsic_redetect, detector_reg, link_cancel_host, link_cwsic_host,
                                      link_ldpc_host, link_mrc_host, link_sic_host, link_sm_host, noise_sigma, sm_weights)
from adafortitran_amd.lmmse import lmmse_estimate_host
from test_linkmrc import MRC_ODD
from test_linksic import _order
from test_linksim import GRIDS, TAU_CAP
from test_linksm import _brute_force, _operands, _rebuilt, sm_cases

PATTERNS = ((0, 0), (1, 0), (0, 1), (1, 1))                  # (failed_0, failed_1): the four a group can be in


def cycled_failed(G):
    """int32 ``[G, 2]``: the four patterns over the groups, a failed stream with a block-error count that varies (any non-zero counts)."""
    f = np.asarray([PATTERNS[g % 4] for g in range(G)], dtype=np.int32)
    return f * (1 + np.arange(G, dtype=np.int32) % 3)[:, None]


def _all(G, s):
    """redo ``[G, 2]`` with stream ``s`` of every group set."""
    redo = np.zeros((G, 2), dtype=bool)
    redo[:, s] = True
    return redo


# ---- cwsic_redetect ----

def test_the_truth_table_of_the_flags():
    assert cwsic_redetect(np.asarray(PATTERNS)).tolist() == [[False, False], [True, False], [False, True], [False, False]]
    assert cwsic_redetect(np.asarray([[3, 0], [0, 7], [2, 5]])).tolist() == [[True, False], [False, True], [False, False]]
    assert cwsic_redetect(np.zeros((2, 3, 2), bool)).shape == (2, 3, 2) and cwsic_redetect(cycled_failed(8)).sum(axis=1).max() == 1
    for bad in (np.zeros(3), np.zeros((4, 3)), np.zeros(())):
        with pytest.raises(ValueError, match="2 streams on its last axis"):
            cwsic_redetect(bad)


# ---- link_cancel_host ----

@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_cancel_twin_is_the_genie_second_stage_exactly(m):
    """Wherever ``link_sic_host(genie=True)`` detects stream s second, ``link_cancel_host``'s LLRs for s with ``redo`` set are equal to
    its LLRs: the same float64 expressions on the same operands.  A stream without ``redo`` is all zeros."""
    for name, R, n in sm_cases():
        for which in ("lmmse", "ideal"):
            sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands(name, R, which)
            cfg, G = LinkConfig(sim, m), n // (2 * R)
            genie = link_sic_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R, tau=TAU_CAP, e_lambda=TAU_CAP, genie=True)
            f = _order(est, rho, R, sim.ofdm)                                    # stream 1 first: stream 0 is the second one
            for s in (0, 1):
                got = link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, R, _all(G, s), tau=TAU_CAP, e_lambda=TAU_CAP)
                second = (f if s == 0 else ~f) & cfg.data_mask
                assert second.any() or name == MRC_ODD
                assert np.array_equal(got[2][:, s][second], genie[2][:, s][second]), (name, R, which, s)
                assert np.array_equal(got[3][:, s][second], genie[4][:, s][second])                 # the wrong-bit maps
                assert np.array_equal(got[4][:, s][second], genie[5][:, s][second])                 # the flags
                own = second & (genie[6] == 0)                                   # at a dependent element the genie's q is q_dep
                assert np.array_equal(got[7][:, s][own], genie[9][:, s][own])                       # q
                for v in got:
                    assert not v[:, 1 - s].any(), (name, R, which, s)
                assert np.array_equal(got[0][:, s, 0], got[3][:, s].sum(axis=(1, 2)))
                assert np.array_equal(got[0][:, s, 1], (got[3][:, s] > 0).sum(axis=(1, 2)))


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_llrs_against_a_brute_force_over_all_symbols_of_the_cancelled_sample(m):
    """``scale g_ss |c / g_ss - a|^2`` over all 2^m symbols, with ``c = m_s - g_so x_o`` rebuilt from the documented streams: pins the
    cancellation, the separable form, the bit order and the scale, to 1e-9 q."""
    for name, R in (("odd_30x7", 2), ("odd_30x7", 3), (MRC_ODD, 2)):
        sim, n, keys, sigma, ideal, est, rho, scale, _ = _operands(name, R, "lmmse", "mmse", 0.01)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        S, T = sim.ofdm
        x, y = _rebuilt(cfg, keys, ideal, sigma, R)
        E = est.astype(np.complex128).reshape(G, R, 2, S, T)
        w = rho.astype(np.float64).reshape(G, R, 2)[:, :, 0, None, None]
        gss = [(w * np.abs(E[:, :, s]) ** 2).sum(1) for s in (0, 1)]
        g01 = (w * E[:, :, 0].conj() * E[:, :, 1]).sum(1)
        ms = [(w * E[:, :, s].conj() * y).sum(1) for s in (0, 1)]
        c = np.stack([ms[0] - g01 * x[:, 1], ms[1] - g01.conj() * x[:, 0]], axis=1)
        p = np.stack(gss, axis=1)
        want = _brute_force(cfg, c / p, scale.astype(np.float64)[:, None, None, None] * p)
        for s in (0, 1):
            out = link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, R, _all(G, s), e_lambda=TAU_CAP)
            llr, q = out[2], out[5]
            assert llr.shape == want.shape == q.shape == (G, 2, S, T, m)
            assert (np.abs(llr - want)[:, s] <= 1e-9 * q[:, s]).all(), (name, R, s)
            assert (q[:, s][..., cfg.data_mask, :] > 0).all() and not q[:, s][..., ~cfg.data_mask, :].any() and not q[:, 1 - s].any()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_an_unheard_other_stream_is_the_diversity_link(m):
    """``H_r1 = E_r1 = 0``: nothing is cancelled, and stream 0 with ``redo`` is ``link_mrc_host`` on the frames (r, 0): counts exactly,
    LLRs to 1e-12 q."""
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, est, rho, scale, _ = _operands(name, R)
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        H, E = ideal.copy(), est.copy()
        H[1::2], E[1::2] = 0, 0
        counts, loss, llr = link_cancel_host(cfg, keys, H, E, sigma, rho, scale, R, _all(G, 0), 2, (1.0, 0.5))
        want = link_mrc_host(cfg, keys[::2], ideal[::2], est[::2], sigma[::2], rho[::2], scale, R, (1.0, 0.5), e_lambda=TAU_CAP)
        assert np.array_equal(counts[:, 0], want[0]) and (np.abs(llr[:, 0] - want[2]) <= 1e-12 * want[5]).all(), (name, R)
        np.testing.assert_allclose(loss[:, 0], want[1], rtol=1e-9, atol=0)
        assert not llr[:, 1].any() and not loss[:, 1].any() and not counts[:, 1].any()


@pytest.mark.parametrize("m", BITS_PER_SYMBOL)
def test_the_exact_extreme(m):
    """The estimates are the channels and there is no noise: the cancelled sample is ``g_ss x_s``, so no bit is wrong at any m and R."""
    for name, R, n in sm_cases():
        sim, n, keys, sigma, ideal, _, rho, scale, _ = _operands(name, R, "ideal")
        cfg, G = LinkConfig(sim, m), n // (2 * R)
        for s in (0, 1):
            counts, loss, llr, wrong, flags = link_cancel_host(cfg, keys, ideal, ideal, np.zeros_like(sigma), rho, scale, R, _all(G, s), tau=0.0)
            assert counts.shape == (G, 2, 2) and counts.dtype == np.int64 and loss.shape == (G, 2, 1) and llr.shape == (G, 2, *sim.ofdm, m)
            assert not counts.any() and not wrong.any() and flags.shape == (G, 2, *sim.ofdm, 2) and llr[:, s][:, cfg.data_mask].all()


def test_what_the_cancel_twin_refuses():
    sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands("odd_30x7", 4)
    cfg, G = LinkConfig(sim, 4), n // 8
    redo = _all(G, 0)
    for bad in (1, 3, 0, 2.0, True, "2"):
        with pytest.raises(ValueError, match="streams"):
            link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, 4, redo, bad)
    for bad in (0, 9, 2.0, -1, True, "2"):
        with pytest.raises(ValueError, match="branches"):
            link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, bad, redo)
    with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
        link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, 1, redo)
    with pytest.raises(ValueError, match="32 frames is not a multiple of branches \\* streams = 3 \\* 2"):
        link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, 3, redo)
    for args, word in (((rho[:8], scale), "rho"), ((rho, scale[:3]), "scale")):
        with pytest.raises(ValueError, match=word):
            link_cancel_host(cfg, keys, ideal, est, sigma, *args, 4, redo)
    for bad in (redo[:3], redo.astype(np.int32), redo.reshape(-1), np.ones((G, 2), bool)):
        with pytest.raises(ValueError, match="redo"):
            link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, 4, bad)
    with pytest.raises(ValueError, match="between 1 and 8 factors"):
        link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, 4, redo, 2, np.ones(9))
    with pytest.raises(ValueError, match="needs an LdpcConfig"):
        link_cwsic_host(CodeConfig(cfg, 64, "1/2"), keys, ideal, est, sigma, rho, scale, reg, 4)


# ---- link_cwsic_host ----

def _small_code(m):
    return LdpcConfig(LinkConfig(GRIDS["odd_30x7"][0], m), (3, 4))               # one block at m = 2, six at m = 8


@pytest.mark.parametrize("m", (2, 8))
def test_the_composition_is_its_parts(m):
    """First-pass counts are ``link_ldpc_host`` on ``link_sm_host``'s LLRs, the flags the truth table on its block errors, the second
    pass ``link_ldpc_host`` on ``link_cancel_host``'s LLRs of the re-detected streams and zeros elsewhere, the final counts step 4."""
    code = _small_code(m)
    cfg = code.link
    for R in (2, 4):
        sim, n, keys, sigma, ideal, est, rho, scale, reg = _operands("odd_30x7", R)
        G = n // (2 * R)
        first, redo, second, final = link_cwsic_host(code, keys, ideal, est, sigma, rho, scale, reg, R)
        sent_keys = np.ascontiguousarray(keys.reshape(G, R, 2)[:, 0, :]).reshape(-1)
        llr = link_sm_host(cfg, keys, ideal, est, sigma, rho, scale, reg, R)[2]
        assert np.array_equal(first.reshape(-1, 3), link_ldpc_host(code, sent_keys, llr.reshape(2 * G, *llr.shape[2:]))[0])
        assert np.array_equal(redo, cwsic_redetect(first[..., 1])) and redo.dtype == np.bool_ and redo.shape == (G, 2)
        again = link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, R, redo)[2]
        whole = link_ldpc_host(code, sent_keys, again.reshape(2 * G, *again.shape[2:]))[0].reshape(G, 2, 3)
        assert np.array_equal(second[redo], whole[redo]) and not second[~redo].any()
        assert np.array_equal(final[..., :2], np.where(redo[..., None], second, first)[..., :2])
        assert np.array_equal(final[..., 2], first[..., 2] + second[..., 2]) and np.array_equal(final, cwsic_final(first, redo, second))
        assert first.dtype == second.dtype == final.dtype == np.int64
        print(f"m = {m}, R = {R}: {int((first[..., 1] > 0).sum())} of {2 * G} streams failed, {int(redo.sum())} detected again, "
              f"{int((redo & (second[..., 1] == 0)).sum())} recovered")


# ---- the accumulator on a CPU device ----

class _Ls(torch.nn.Module):
    def __init__(self, sim):
        super().__init__()
        self.sim = sim

    def forward(self, pilots):
        return torch.from_numpy(ls_interpolate(self.sim, pilots.cpu().numpy()))


def _sweep(seed, err_var, R):
    """(code, batches with the LS estimate, the recomputation from the definition batch by batch): odd_30x7, QPSK, the (3, 4) code."""
    code = _small_code(2)
    sim = code.link.sim
    model = _Ls(sim)
    batches = [(model(p), ideal, meta) for p, ideal, meta in SynthLoader(sim, 8, 32, device="cpu", seed=seed)]
    want = dict(first=np.zeros(3, np.int64), final=np.zeros(3, np.int64), again=0, decoded=0, both=0, rows=0)
    for est, ideal, meta in batches:
        keys = frame_keys(seed, np.rint(meta[0].numpy().reshape(-1)).astype(np.int64))
        snr = meta[1].numpy().reshape(-1)
        rho, scale, reg = sm_weights(snr, err_var, R, 2, "mmse")
        first, redo, second, final = link_cwsic_host(code, keys, ideal.numpy(), est.numpy(), noise_sigma(snr), rho, scale, reg, R)
        want["first"] += first.sum(axis=(0, 1))
        want["final"] += final.sum(axis=(0, 1))
        want["again"] += int(redo.sum())
        want["decoded"] += int((redo & (second[..., 1] == 0)).sum())
        want["both"] += int((first[..., 1] > 0).all(axis=1).sum())
        want["rows"] += redo.size
    return code, batches, want


def _check(acc, mmse, code, want):
    F, B = want["rows"], code.blocks
    assert acc.frames == mmse.frames == F and acc.detector == "cwsic" and acc.errors.dtype == torch.int64
    assert acc.result_first_pass() == mmse.result() == want["first"][1] / (F * B)           # exactly the MMSE sweep's
    assert acc.errors.tolist() == want["final"].tolist() and acc._first.tolist() == mmse.errors.tolist() == want["first"].tolist()
    assert acc.result() == want["final"][1] / (F * B) and acc.result_ber() == want["final"][0] / (F * code.info_bits_per_frame)
    assert acc.result_throughput() == (F * B - want["final"][1]) * code.info_bits / (F * code.link.data_elements)
    assert acc.result_iterations() == want["final"][2] / (F * B) >= mmse.result_iterations()
    assert acc.cwsic_stats() == (want["again"] / F, want["decoded"] / want["again"] if want["again"] else 0.0, want["both"] / (F // 2))


def test_the_accumulator_on_a_cpu_device_is_the_definition_batch_by_batch():
    from adafortitran_amd.evaluation import get_link_bler
    seed, err_var, R = 5, 0.01, 2
    code, batches, want = _sweep(seed, err_var, R)
    acc = LdpcBlockErrorAccumulator(code, "cpu", seed, err_var, R, 2, "cwsic")
    mmse = LdpcBlockErrorAccumulator(code, "cpu", seed, err_var, R, 2, "mmse")
    for est, ideal, meta in batches:
        acc.update(est, ideal, meta)
        mmse.update(est, ideal, meta)
    assert want["again"] > 0 and 0 < want["first"][1]                            # the sweep re-detects something: not vacuous
    _check(acc, mmse, code, want)
    acc.update(est[:0], ideal[:0], meta)                                         # an empty batch changes nothing
    _check(acc, mmse, code, want)
    empty = LdpcBlockErrorAccumulator(code, "cpu", seed, err_var, R, 2, "cwsic")
    assert empty.result() == empty.result_first_pass() == 0.0 and empty.cwsic_stats() == (0.0, 0.0, 0.0)
    loaders = [("SNR_0", SynthLoader(code.link.sim, 8, 32, device="cpu", seed=seed, fresh_each_epoch=False))]
    assert get_link_bler(_Ls(code.link.sim), loaders, code, seed, err_var, branches=R, streams=2, detector="cwsic") == {0: acc.result()}
    for other in (mmse, LdpcBlockErrorAccumulator(code, "cpu", seed, err_var, R, 2, "sic")):
        for read in (other.result_first_pass, other.cwsic_stats):
            with pytest.raises(ValueError, match='needs streams=2 and detector="cwsic"'):
                read()


def _rank(rank, world, port, seed, err_var, R, out):
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        code, batches, _ = _sweep(seed, err_var, R)
        acc = LdpcBlockErrorAccumulator(code, "cpu", seed, err_var, R, 2, "cwsic")
        for est, ideal, meta in batches[rank::world]:
            acc.update(est, ideal, meta)
        out.put((rank, acc.result(), acc.result_ber(), acc.result_throughput(), acc.result_iterations(), acc.result_first_pass(),
                 acc.cwsic_stats()))
    finally:
        dist.destroy_process_group()


def test_two_ranks_give_the_one_rank_result():
    import torch.multiprocessing as mp
    seed, err_var, R = 5, 0.01, 2
    code, batches, want = _sweep(seed, err_var, R)
    one = LdpcBlockErrorAccumulator(code, "cpu", seed, err_var, R, 2, "cwsic")
    for est, ideal, meta in batches:
        one.update(est, ideal, meta)
    alone = (one.result(), one.result_ber(), one.result_throughput(), one.result_iterations(), one.result_first_pass(), one.cwsic_stats())
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, seed, err_var, R, out)) for r in range(2)]
    for p in procs:
        p.start()
    got = [out.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert sorted(g[0] for g in got) == [0, 1] and all(tuple(g[1:]) == alone for g in got)


# ---- refusals ----

def test_cwsic_is_refused_wherever_no_ldpc_decoder_runs():
    from adafortitran_amd.evaluation import get_link_rates, get_link_stats
    sim = GRIDS["odd_30x7"][0]
    cfg = LinkConfig(sim, 2)
    ldpc, conv = LdpcConfig(cfg, (3, 4)), CodeConfig(cfg, 64, "1/2")
    instead = "LdpcBlockErrorAccumulator"
    for make in (lambda: LinkAccumulator(cfg, "cpu", branches=2, streams=2, detector="cwsic"),
                 lambda: RateAccumulator(cfg, "cpu", branches=2, streams=2, detector="cwsic"),
                 lambda: BlockErrorAccumulator(conv, "cpu", branches=2, streams=2, detector="cwsic"),
                 lambda: HarqAccumulator(HarqConfig(ldpc, 4, 2), "cpu", detector="cwsic"),
                 lambda: LinkAccumulator(cfg, "cpu", detector="cwsic"),
                 lambda: get_link_stats(None, [], cfg, branches=2, streams=2, detector="cwsic"),
                 lambda: get_link_rates(None, [], cfg, branches=2, streams=2, detector="cwsic")):
        with pytest.raises(ValueError, match=f'has no detector="cwsic".*{instead}'):
            make()
    for kw in (dict(streams=1), dict(streams=1, branches=2), dict(streams=1, branches=2, tx_diversity="time"),
               dict(streams=1, branches=2, precoding_subband=6)):
        with pytest.raises(ValueError, match='detector="cwsic" cancels one of 2 spatial streams.*use detector="mmse"'):
            LdpcBlockErrorAccumulator(ldpc, "cpu", detector="cwsic", **kw)
    with pytest.raises(ValueError, match="one antenna cannot separate 2 streams"):
        LdpcBlockErrorAccumulator(ldpc, "cpu", streams=2, detector="cwsic")
    with pytest.raises(ValueError, match="6 frames is not a multiple of branches \\* streams = 2 \\* 2"):
        LdpcBlockErrorAccumulator(ldpc, "cpu", branches=2, streams=2, detector="cwsic").update(
            None, torch.zeros((6, *sim.ofdm), dtype=torch.complex64), frame_ids=np.arange(6), snr_db=np.zeros(6))
    with pytest.raises(TypeError, match="unexpected keyword argument 'streams'"):
        HarqAccumulator(HarqConfig(ldpc, 4, 2), "cpu", streams=2)
    for bad in ("cwsic", "ml"):                                                  # the regulariser stays the linear detectors'
        with pytest.raises(ValueError, match="detector"):
            detector_reg(np.ones(2, np.float32), bad)
    for bad in ("CWSIC", "cw-sic", None):
        with pytest.raises(ValueError, match="detector"):
            LdpcBlockErrorAccumulator(ldpc, "cpu", branches=2, streams=2, detector=bad)


# ---- pinned constants ----

def test_the_entry_points_are_in_the_signature_table_and_the_abi_version_stays():
    assert _abi.AFT_ABI_VERSION == 10
    assert DETECTORS == ("zf", "mmse") and ALL_DETECTORS == ("zf", "mmse", "joint") and LINK2_DETECTORS == ("zf", "mmse", "joint", "sic")
    assert linksim.CWSIC_DETECTOR == "cwsic" and linksim.CODED_DETECTORS == LINK2_DETECTORS + ("cwsic",)
    sm, ldpc = _abi.SIGNATURES["aft_link_sm_f32"][1], _abi.SIGNATURES["aft_link_ldpc_f32"][1]
    restype, argtypes = _abi.SIGNATURES["aft_link_cancel_f32"]
    # aft_link_sm_f32's list less reg, with failed and its stride in front of counts and state behind llr
    assert restype is C.c_int and argtypes == sm[:7] + sm[8:12] + [C.c_void_p, C.c_int] + sm[12:15] + [C.c_void_p] + sm[15:]
    restype, argtypes = _abi.SIGNATURES["aft_link_ldpc_masked_f32"]
    assert restype is C.c_int and argtypes == ldpc[:11] + [C.c_void_p, C.c_int] + ldpc[11:]      # the mask and its stride in front of counts
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "adafortitran_amd.h")).read()
    declared = re.findall(r"^(?:int|size_t|const char \*)\s*(aft_\w+)\(", header, flags=re.M)
    names = list(_abi.SIGNATURES)
    for name in ("aft_link_cancel_f32", "aft_link_ldpc_masked_f32"):
        assert name in _abi.EXPORTED_SYMBOLS and declared.count(name) == 1 and declared.index(name) == names.index(name)
    assert names.index("aft_link_cancel_f32") == names.index("aft_link_sic_f32") + 1 == names.index("aft_link_ldpc_masked_f32") - 1


# ---- physical conditions ----

PHYSICAL = dict(bits=2, rate="1/2", branches=2, snr_db=10.0, delay_spread_ns=200.0, doppler_hz=800.0, frames=128, pack_seed=110, key_seed=1)
_physical = {}


def physical_inputs():
    """QPSK, LDPC rate 1/2, 2 x 2, 10 dB, 200 ns, 800 Hz, 128 frames of ``make_pack(seed=110)``, seed-1 keys: ``(code, keys, sigma,
    snr, ideal, {"perfect", "lmmse", "ls"})``, made once and read-only; tests/test_linkcwsic_gpu.py runs the device on the same arrays."""
    if not _physical:
        p = PHYSICAL
        sim = ChannelSimConfig()
        pack = make_pack(sim, p["frames"], seed=p["pack_seed"], snr_db=p["snr_db"], delay_spread_ns=p["delay_spread_ns"], doppler_hz=p["doppler_hz"])
        ideal, snr = pack["h_ideal"], pack["meta"][:, 1].astype(np.float64)
        pilots = pack["h_ls_sparse"][:, np.asarray(sim.pilot_scs)][:, :, np.asarray(sim.pilot_symbols)]
        est = {"perfect": ideal, "lmmse": lmmse_estimate_host(sim, pilots, pack["meta"][:, 1:4]).astype(np.complex64), "ls": pack["h_ls_full"]}
        keys, sigma = frame_keys(p["key_seed"], np.arange(p["frames"])), noise_sigma(snr)
        for a in (ideal, keys, sigma, snr, *est.values()):
            a.setflags(write=False)
        _physical["inputs"] = (LdpcConfig(LinkConfig(sim, p["bits"]), p["rate"]), keys, sigma, snr, ideal, est)
    return _physical["inputs"]


def physical_conditions(counts):
    """The conditions of the issue on ``{estimator: (first, redo, second, final)}``, whoever computed the counts: at least 4 streams are
    re-detected with LMMSE, at least one of them is recovered and at least one is not; with perfect CSI every re-detected stream is
    recovered; BLER after <= BLER before for all three; the recovered share orders perfect >= LMMSE >= LS."""
    share = {}
    for which, (first, redo, second, final) in counts.items():
        again, recovered = int(redo.sum()), int((redo & (second[..., 1] == 0)).sum())
        share[which] = recovered / again if again else 1.0
        before, after = int(first[..., 1].sum()), int(final[..., 1].sum())
        print(f"{which}: {redo.size} streams, {int((first[..., 1] > 0).sum())} failed the first pass, {int((first[..., 1] > 0).all(axis=1).sum())} "
              f"groups both, {again} detected again, {recovered} recovered; block errors {before} -> {after}")
        assert after <= before, which
        if which == "lmmse":
            assert again >= 4 and 1 <= recovered < again
        if which == "perfect":
            assert recovered == again
    assert share["perfect"] >= share["lmmse"] >= share["ls"], share


def test_physical_conditions_on_the_twin():
    code, keys, sigma, snr, ideal, est = physical_inputs()
    rho, scale, reg = sm_weights(snr, 0.0, PHYSICAL["branches"], 2, "mmse")
    physical_conditions({which: link_cwsic_host(code, keys, ideal, e, sigma, rho, scale, reg, PHYSICAL["branches"]) for which, e in est.items()})
    # at rate 1/2 the channel itself leaves nothing to detect again; at rate 3/4 it does, so that condition is not vacuous
    first, redo, second, final = link_cwsic_host(LdpcConfig(code.link, "3/4"), keys, ideal, ideal, sigma, rho, scale, reg, PHYSICAL["branches"])
    again, recovered = int(redo.sum()), int((redo & (second[..., 1] == 0)).sum())
    print(f"perfect, rate 3/4: {again} detected again, {recovered} recovered; block errors {int(first[..., 1].sum())} -> {int(final[..., 1].sum())}")
    assert again >= 1 and recovered == again and final[..., 1].sum() <= first[..., 1].sum()
