"""Evaluation sweep without per-batch host syncs.

Mirrors ``ModelEvaluator._evaluate_dataloader`` / ``get_test_stats`` of the reference
(src/main/trainer.py:311-347): same dispatch on the estimator class, same sample-weighted mean of
``2 * MSELoss(cat(Re, Im))`` per loader, same ``{int(val): dB}`` dictionary sorted by the integer in
the loader's name -- but the squared error accumulates on the device (metrics.MseAccumulator) and is
read back once per loader (plus one all-gather when several ranks each evaluate a shard).

With an ``ingest.PackedLoader`` on a HIP device the reference's pilot-count ``ValueError`` ("Expected 24 pilot values, got 25",
dataset.py:128-132) surfaces ONE BATCH LATE -- while the next batch is prepared, at the end of the sweep, or when the iterator is
closed early -- because the counts come back asynchronously; the sweep therefore never returns a value computed from a bad frame
without raising, but the exception's traceback points at the loader, not at the forward of the offending batch."""
from __future__ import annotations

import itertools
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from .estimators import AdaFortiTranEstimator
from .linksim import (DEFAULT_FACTORS, BlockErrorAccumulator, HarqAccumulator, LdpcBlockErrorAccumulator, LdpcConfig, LinkAccumulator,
                      RateAccumulator, _refuse_cwsic, as_refiner)
from .lmmse import LmmseEstimator
from .metrics import MseAccumulator, to_db


def forward_pass(model: torch.nn.Module, pilots: torch.Tensor, meta_data: Optional[tuple]) -> torch.Tensor:
    """The reference's ``_forward_pass`` (trainer.py:267-288): AdaFortiTran needs ``meta_data``; the LMMSE baseline takes it too (its
    design point per frame), and may do without when every condition is pinned."""
    if isinstance(model, LmmseEstimator):
        return model(pilots, meta_data)
    if isinstance(model, AdaFortiTranEstimator):
        if meta_data is None:
            raise ValueError("AdaFortiTranEstimator requires meta_data but it was not provided")
        return model(pilots, meta_data)
    return model(pilots)


def evaluate_dataloader(model: torch.nn.Module, dataloader: Iterable, group=None) -> float:
    """Mean |h_est - h|^2 over every complex element of the loader (one host sync at the end)."""
    model.eval()
    device = next(itertools.chain(model.parameters(), model.buffers())).device      # the LMMSE baseline has buffers only
    acc = MseAccumulator(device)
    with torch.no_grad():
        for pilots, ideal, meta in dataloader:
            acc.update(forward_pass(model, pilots, meta), ideal)
    return acc.result(group)


def get_test_stats(model: torch.nn.Module, test_dataloaders: List[Tuple[str, Iterable]], group=None) -> Dict[int, float]:
    stats: Dict[int, float] = {}
    for name, loader in sorted(test_dataloaders, key=lambda x: int(x[0].split("_")[1])):
        stats[int(name.split("_")[1])] = to_db(evaluate_dataloader(model, loader, group))
    return stats


def _link_sweep(model, test_dataloaders, make_acc, read, make_refiner=None) -> Dict[int, float]:
    """One accumulator per loader, sorted and keyed as ``get_test_stats``: ``make_acc(device)`` opens it, ``read(acc)`` closes it.
    ``make_refiner(device)``, where given, returns None or the ``linksim.DataAidedRefiner`` whose ``refine`` runs between the
    estimator and the accumulator (one per sweep: a refiner that was handed in keeps counting over the loaders)."""
    if model is not None:
        model.eval()
    stats: Dict[int, float] = {}
    refiner = None
    for name, loader in sorted(test_dataloaders, key=lambda x: int(x[0].split("_")[1])):
        acc = None
        with torch.no_grad():
            for pilots, ideal, meta in loader:
                est = None if model is None else forward_pass(model, pilots, meta)
                if acc is None:
                    acc = make_acc(ideal.device if est is None else est.device)
                    if make_refiner is not None and refiner is None:
                        refiner = make_refiner(acc.device)
                if refiner is not None:
                    est = refiner.refine(est, pilots, ideal, meta)
                acc.update(est, ideal, meta)
        if acc is None:
            raise ValueError(f"loader {name} yielded no batch")
        stats[int(name.split("_")[1])] = read(acc)
    return stats


class _MseOfSweep(MseAccumulator):
    """``MseAccumulator`` with the ``update(est, ideal, meta)`` of the link accumulators, for ``_link_sweep``."""

    def update(self, est, ideal, meta=None) -> None:
        super().update(est, ideal)


def _refiner_maker(refine, link_cfg, seed, branches, streams=1, tx_diversity=None, precoding_subband=None, err_var=0.0):
    """``refine=`` of a sweep -> None (the sweep as it was, launch for launch) or ``device -> DataAidedRefiner``; what
    ``linksim.as_refiner`` refuses is refused here, before the first batch."""
    if refine is None:
        return None
    as_refiner(refine, link_cfg, None, seed, branches, streams, tx_diversity, precoding_subband, err_var)
    return lambda device: as_refiner(refine, link_cfg, device, seed, branches, streams, tx_diversity, precoding_subband, err_var)


def get_link_stats(model: Optional[torch.nn.Module], test_dataloaders: List[Tuple[str, Iterable]], link_cfg, seed: int = 0,
                   group=None, branches: int = 1, streams: int = 1, detector: str = "mmse",
                   tx_diversity: Optional[str] = None, precoding_subband: Optional[int] = None, precoding_delay: int = 0,
                   slots: int = 1, refine=None) -> Dict[int, float]:
    """Bit-error rate per loader on the link ``link_cfg`` (``linksim.LinkConfig``) defines: data symbols through each frame's true channel
    plus noise at the frame's SNR, equalised with the model's estimate; ``model=None`` is perfect channel knowledge.  Same sorting and
    keys as ``get_test_stats``; the estimate comes from ``forward_pass``, so every estimator here works; the counts accumulate on the
    device (``linksim.LinkAccumulator``) and are read once per loader.  A frame's data bits and noise are a function of
    ``(seed, file_no)``, whichever estimator is measured: two estimators see the same link.
    ``branches=R`` combines every R consecutive frames of a batch as the antennas of one receiver (``linksim``: "the diversity link");
    every batch then holds a multiple of R frames.  ``streams=2`` with ``detector`` ``"zf"`` or ``"mmse"`` separates two transmit
    streams on those R antennas (``linksim``: "the spatial-multiplexing link"): every batch holds a multiple of ``2 R`` frames, frame
    ``r 2 + s`` of a group the pair (antenna r, stream s), and the rate is per stream.  ``detector="joint"`` runs the joint max-log
    demapper on the same frames instead of a linear detector (``linksim``: "the joint link"), ``detector="sic"`` ordered MMSE-SIC
    (``linksim``: "the successive-cancellation link").  ``tx_diversity="time"`` or
    ``"frequency"`` sends ONE stream from two transmit antennas as Alamouti pairs over adjacent data symbols or subcarriers
    (``linksim``: "the transmit-diversity link"): every batch holds a multiple of ``2 R`` frames in the same order, ``streams`` must
    be 1, ``detector`` is ignored, and the SNR is per transmit antenna.  ``precoding_subband=B`` sends ONE stream from the same two
    antennas co-phased by a codebook precoder picked per subband of ``B`` subcarriers from the estimate (``linksim``: "the closed-loop
    link"): the same groups of ``2 R`` frames, ``streams`` must be 1 and ``tx_diversity`` None.  ``precoding_delay=d`` with ``slots=K``
    applies PMIs selected ``d`` slots earlier on loaders of ``ChannelSimConfig(slots=K)`` (``linksim``: "delayed feedback"): every batch
    holds whole sequences of ``K 2 R`` frames, and the rate counts the transmitted slots only.  ``detector="cwsic"`` is refused: no
    decoder runs here (``get_link_bler`` with an ``LdpcConfig`` has it).
    ``refine=`` (the same keyword on ``get_link_rates``, ``get_link_bler`` and ``get_link_harq``; None, the default, is the sweep as it
    was, launch for launch): an iteration count or a ``linksim.DataAidedRefiner`` -- the estimate is refined from the receiver's own
    hard decisions (``linksim``: "the decision-directed observation") on the very received samples the accumulator then measures,
    and the rate is that of the REFINED estimate.  One transmit stream only: with ``streams=2``, ``tx_diversity`` or
    ``precoding_subband`` it is refused (``branches=R`` works); ``model=None`` has nothing to refine."""
    _refuse_cwsic(detector, "get_link_stats", 'detector="sic" is the symbol-level cancellation it runs')
    return _link_sweep(model, test_dataloaders,
                       lambda device: LinkAccumulator(link_cfg, device, seed, branches, streams, detector, tx_diversity=tx_diversity,
                                                      precoding_subband=precoding_subband, precoding_delay=precoding_delay, slots=slots),
                       lambda acc: acc.result(group),
                       _refiner_maker(refine, link_cfg, seed, branches, streams, tx_diversity, precoding_subband))


def get_link_rates(model: Optional[torch.nn.Module], test_dataloaders: List[Tuple[str, Iterable]], link_cfg, seed: int = 0,
                   factors=DEFAULT_FACTORS, group=None, branches: int = 1, streams: int = 1, detector: str = "mmse",
                   tx_diversity: Optional[str] = None, precoding_subband: Optional[int] = None, precoding_delay: int = 0,
                   slots: int = 1, refine=None) -> Dict[int, float]:
    """Achievable rate per loader in bit/symbol on the same link: the bit-interleaved coded-modulation rate (GMI) of the max-log LLRs a
    demapper forms with the model's estimate at the frame's SNR, the best of the LLR scale factors ``factors``; ``model=None`` is perfect
    channel knowledge.  Sorting, keys and the frames' bits and noise as ``get_link_stats``; the losses accumulate on the device
    (``linksim.RateAccumulator``) and are read once per loader.  ``branches``, ``streams`` and ``detector`` as ``get_link_stats``: the rate is per
    transmission, with two streams per stream and symbol (the spectral efficiency is twice it).  ``tx_diversity`` as
    ``get_link_stats``: the rate of the one stream the two antennas send; ``precoding_subband``, ``precoding_delay`` and ``slots``
    likewise.  ``detector="cwsic"`` is refused, as by ``get_link_stats``.  ``refine`` as ``get_link_stats``."""
    _refuse_cwsic(detector, "get_link_rates", 'detector="sic" is the symbol-level cancellation it runs')
    return _link_sweep(model, test_dataloaders, lambda device: RateAccumulator(link_cfg, device, seed, factors, branches=branches,
                                                                               streams=streams, detector=detector,
                                                                               tx_diversity=tx_diversity,
                                                                               precoding_subband=precoding_subband,
                                                                               precoding_delay=precoding_delay, slots=slots),
                       lambda acc: acc.result_gmi(group),
                       _refiner_maker(refine, link_cfg, seed, branches, streams, tx_diversity, precoding_subband))


def get_link_bler(model: Optional[torch.nn.Module], test_dataloaders: List[Tuple[str, Iterable]], code_cfg, seed: int = 0,
                  err_var: float = 0.0, group=None, branches: int = 1, streams: int = 1, detector: str = "mmse",
                  tx_diversity: Optional[str] = None, precoding_subband: Optional[int] = None, precoding_delay: int = 0,
                  slots: int = 1, refine=None) -> Dict[int, float]:
    """Block-error rate per loader with a decoder in the loop: the code ``code_cfg`` rides on the same link and its decoder reads the
    max-log LLRs the demapper forms with the model's estimate -- a ``linksim.CodeConfig`` is the convolutional code with a Viterbi
    decoder (``linksim.BlockErrorAccumulator``), a ``linksim.LdpcConfig`` the quasi-cyclic LDPC code with a layered min-sum decoder
    (``linksim.LdpcBlockErrorAccumulator``); ``model=None`` is perfect channel knowledge.  Sorting, keys and the frames' bits and noise
    as ``get_link_stats``; the counts accumulate on the device and are read once per loader.  ``branches`` as ``get_link_stats``: the
    decoder reads the combiner's LLRs with the leaders' keys; ``streams`` and ``detector`` likewise: the decoder reads each stream's
    LLRs with the key of frame ``(0, s)``; ``tx_diversity`` as ``get_link_stats``: the decoder reads the Alamouti combiner's LLRs with
    the leaders' keys; ``precoding_subband`` likewise, on the closed-loop link's LLRs, and with ``precoding_delay`` and ``slots`` on
    the transmitted slots' LLRs with the transmit slots' leader keys.  ``detector="cwsic"`` with ``streams=2`` and an
    ``LdpcConfig`` is codeword-level cancellation (``linksim``: "the codeword-cancellation link"): the rate returned is the one AFTER
    the second pass; an accumulator of one's own (``LdpcBlockErrorAccumulator``) also reads ``result_first_pass`` and ``cwsic_stats``.
    ``refine`` as ``get_link_stats``, on the link of ``code_cfg``; with several branches the refiner combines with this ``err_var``'s
    weights, the accumulator's own."""
    accumulator = LdpcBlockErrorAccumulator if isinstance(code_cfg, LdpcConfig) else BlockErrorAccumulator
    return _link_sweep(model, test_dataloaders,
                       lambda device: accumulator(code_cfg, device, seed, err_var, branches, streams, detector, tx_diversity=tx_diversity,
                                                  precoding_subband=precoding_subband, precoding_delay=precoding_delay, slots=slots),
                       lambda acc: acc.result(group),
                       _refiner_maker(refine, code_cfg.link, seed, branches, streams, tx_diversity, precoding_subband, err_var))


def get_link_harq(model: Optional[torch.nn.Module], test_dataloaders: List[Tuple[str, Iterable]], harq_cfg, seed: int = 0,
                  err_var: float = 0.0, group=None, branches: int = 1, refine=None) -> Dict[int, float]:
    """Throughput per loader under hybrid ARQ, in delivered information bits per data element sent (``linksim``: "The HARQ link"):
    ``harq_cfg`` (``linksim.HarqConfig``) rate-matches an LDPC mother code, every ``rounds`` consecutive frames of a batch -- after the
    combiner, with ``branches`` -- are the transmission rounds of one set of blocks, and a block is sent again until it decodes;
    ``model=None`` is perfect channel knowledge.  Sorting, keys and the frames' bits and noise as ``get_link_stats``; the counts
    accumulate on the device (``linksim.HarqAccumulator``) and are read once per loader.  Every batch holds a multiple of
    ``branches * rounds`` frames.  ``refine`` as ``get_link_stats``, on the link of ``harq_cfg``."""
    return _link_sweep(model, test_dataloaders, lambda device: HarqAccumulator(harq_cfg, device, seed, err_var, branches),
                       lambda acc: acc.result_throughput(group), _refiner_maker(refine, harq_cfg.link, seed, branches, err_var=err_var))


def get_refined_test_stats(model: torch.nn.Module, test_dataloaders: List[Tuple[str, Iterable]], link_cfg, refine=1, seed: int = 0,
                           group=None, branches: int = 1) -> Dict[int, float]:
    """``get_test_stats`` of the REFINED estimate: per loader the mean ``|h_est' - h|^2`` in dB (the NMSE: ``E|H|^2 = 1``) of what
    ``refine`` -- an iteration count or a ``linksim.DataAidedRefiner``, as in ``get_link_stats`` -- makes of the model's estimate on
    the link ``link_cfg`` with the frames' bits and noise of ``seed``.  Same sorting and keys; the squared error accumulates on the
    device and is read once per loader.  ``refine=0`` is ``get_test_stats`` itself."""
    make = _refiner_maker(refine, link_cfg, seed, branches)
    if make is None:
        raise ValueError("refine = None: an iteration count or a DataAidedRefiner (get_test_stats measures the unrefined estimate)")
    return _link_sweep(model, test_dataloaders, _MseOfSweep, lambda acc: to_db(acc.result(group)), make)
