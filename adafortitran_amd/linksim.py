"""Link-level bit errors: what a channel estimate is worth to the receiver that uses it.

Every comparison of estimators here ends in channel MSE.  A receiver uses the estimate to equalise data symbols, so the first question
about an MSE gain is how many bit errors it removes, at which modulation order and SNR.  This module DEFINES the link: data symbols
through the TRUE channel plus noise, a one-tap equaliser that uses the ESTIMATE, a hard demapper and a bit-error count, as a pure
function of the frame's key, its noise scale, its true channel and the estimate:

* ``link_errors_host`` evaluates the definition in float64 with NumPy -- the CPU path and the yardstick;
* ``aft_link_errors_f32`` (csrc/k_link.hip, through ``hip_ops.LinkPlan``) evaluates it in float32 on the device, one launch per batch;
* ``LinkAccumulator`` sums a sweep's counts the way ``metrics.MseAccumulator`` sums squared errors; ``evaluation.get_link_stats`` is the
  sweep.

The definition.  For a frame: key ``kf`` (64 bits; for simulated frames ``chansim.frame_keys(seed, g)``, the simulator's own), true channel
``H`` and estimate ``E`` (complex64 ``[S, T]``), noise scale ``sigma`` (float32), ``m`` bits per symbol in {2, 4, 6, 8} (square QAM),
``L = 2^(m/2)`` levels per axis, ``d = sqrt(3 / (2 (L^2 - 1)))`` (unit mean symbol energy).  Over every grid element ``(s, t)`` that is
not a pilot position (``pilot_scs x pilot_symbols`` of the ``ChannelSimConfig``), ``q = s T + t``::

    word(stream, q) = splitmix64(kf ^ (stream << 32 | q))       streams 5 data bits, 6 data-noise radius, 7 data-noise angle
    w  = word(5, q) >> (64 - m),   gi = w >> (m/2),   gq = w & (L - 1)            the sent Gray codes of the I and the Q axis
    k  : k ^ (k >> 1) = g                                                          the level index of a Gray code
    x  = d ((2 ki - (L-1)) + j (2 kq - (L-1)))                                     the sent symbol
    y  = H[s,t] x + sigma sqrt(-ln u1) exp(j 2 pi u2)                              u = ((word >> 41) + 0.5) 2^-23 of streams 6 and 7
    c  = y conj(E[s,t]),   p = |E[s,t]|^2
    k^ = #{b in 1 .. L-1 : comp >= beta_b p},   beta_b = 2 d (b - L/2)             per axis, comp = Re c for I and Im c for Q
    bit errors    = sum popcount(gi ^ g^i) + popcount(gq ^ g^q),   g^ = k^ ^ (k^ >> 1)
    symbol errors = the number of elements with any bit wrong

This is zero-forcing with a hard decision and without a division: a total function with no special case for ``p = 0``.  The noise is the
simulator's Box-Muller (the angle is formed in turns and reduced before its sine and cosine); streams 0-4 stay the simulator's.  A frame
carries ``m (S T - Ps Pt)`` bits.  ``sigma`` for a frame at ``snr_db`` is ``float32(10^(-snr_db / 20))``, formed in double and rounded
once (``noise_sigma``; the rule of ``ChannelSimConfig.tables()["noise_sigma"]``).

The margin, which is what a float32 evaluation is compared through: for each (element, axis, boundary)
``|comp - beta_b p| / ((|H||x| + |noise|) |E| + |beta_b| p)``, 0 where the denominator is 0.  An (element, axis) is FLAGGED at ``tau``
when any of its boundaries has margin <= ``tau``: there a relative error of ``tau`` in the two sides may move the decision across that
boundary.  Because of the Gray map a flagged (element, axis) changes a frame's bit-error count by at most 1, and a
flagged element its symbol-error count by at most 1.

The soft link.  No OFDM system runs uncoded 64- or 256-QAM: what decides whether an MSE gain matters is how much soft information the
demapper hands the decoder.  The decoder-free measure of that is the bit-interleaved coded-modulation rate, the generalised mutual
information (GMI) of the LLRs.  ``link_llrs_host`` (float64), ``aft_link_soft_f32`` (csrc/k_link.hip, through ``hip_ops.LinkSoftPlan``),
``RateAccumulator`` and ``evaluation.get_link_rates`` are to it what the four names above are to the bit errors.  Per frame and data
element, with ``w, gi, gq, x, y, c, p`` exactly as above::

    levels   a_k = d (2k - (L-1)),  label g_k = k ^ (k >> 1),  k = 0 .. L-1
    metric   mu_k(comp) = a_k (a_k p - 2 comp)        |y - E x|^2 up to a constant, separable per axis, no division
    bit j of an axis's Gray code, MSB first:  bit_j(g) = (g >> (m/2 - 1 - j)) & 1
    Delta_j  = min{mu_k : bit_j(g_k) = 1} - min{mu_k : bit_j(g_k) = 0}
    LLR      Lambda_j = scale Delta_j                 positive favours bit 0; I-axis bits 0 .. m/2-1, Q-axis bits m/2 .. m-1 (the order of w)
    loss_f  += log2(1 + exp(-(1 - 2 b_j) factor_f Lambda_j))       b_j the sent bit, for each of the K factors

``scale`` is a float32 per frame (``llr_scale``: one over the noise variance plus the estimate's error variance), ``factors`` float32
``[K]``, 1 <= K <= 8.  The LLR at a pilot position is 0.  A frame's rate at factor f is ``m - loss_f / data_elements`` bit/symbol; it
may be negative (over-confident LLRs under a mismatched channel, which is why the loss is evaluated on a grid of factors in one pass),
and the best of the grid is the GMI's supremum over the LLR scale taken on that grid.

What a float32 evaluation of the LLRs is compared through: ``q = scale A (A p + 2 R)`` with ``A = (L-1) d`` the outermost level and
``R = (|H||x| + |noise|) |E|`` the reach of ``comp`` -- every ``|mu_k| <= A (A p + 2 R)``, so an evaluation whose metrics err by a
relative ``e`` of that errs in ``Lambda_j`` by about ``2 e q``.  The loss is monotone in every ``Lambda_j``, so the losses at
``Lambda -+ e_lambda q`` (each bit moved towards, or away from, the sent bit) are an exact interval for every evaluation whose LLRs
are within ``e_lambda q``.

The diversity link.  Every number above is a single-antenna Rayleigh number: at the SNRs where 64- and 256-QAM operate such a link
loses its blocks to deep fades of the true channel, not to the estimate.  Receivers have two or four antennas, each with its own
channel estimate, combined before the demapper.  ``link_mrc_host`` (float64), ``aft_link_mrc_f32`` (csrc/k_link.hip, through
``hip_ops.LinkMrcPlan``) and the ``branches=`` argument of the four accumulators and of the three sweeps of ``evaluation`` are maximum-
ratio combining over R branches.  The estimators here are per-antenna by construction -- one frame is one antenna's grid -- so a batch
of ``n`` frames with ``R = branches``, ``1 <= R <= 8`` and ``n % R == 0``, is ``G = n / R`` groups: group ``g`` is the frames
``g R .. g R + R - 1``, its branches ``r = 0 .. R-1``, branch 0 its LEADER::

    w, gi, gq, x   from the leader's key exactly as above (stream 5): one transmission per group; stream 5 of the other keys is unused
    y_r  = H_r x + sigma_r sqrt(-ln u1) exp(j 2 pi u2)          u1, u2 from streams 6 and 7 of branch r's OWN key, sigma_r that frame's
    c    = sum_r rho_r y_r conj(E_r),   p = sum_r rho_r |E_r|^2     summed in increasing r, starting from 0
    rho_r = float32(scale_r / scale_leader)                      scale_* = llr_scale(snr, err_var) of the frame; the ratio is formed in
                                                                 double and rounded once, so rho_0 = 1 exactly (``branch_weights``)

This is maximum-ratio combining with per-branch noise variances and still has no division on the device; all ``rho`` are 1 when the
branches share an SNR.  The hard decision, the bit and symbol errors, ``mu_k``, ``Delta_j``, ``Lambda_j = scale Delta_j`` with the
LEADER's scale (one float32 per group) and the losses at the K factors are the single-branch definitions applied to this ``c`` and
``p``, per group: counts ``[G, 2]``, loss ``[G, K]``, llr ``[G, S, T, m]``.  With ``R = 1`` every output is the single-branch one.  The
margin and the LLR reach use ``reach = sum_r rho_r (|H_r||x| + |noise_r|) |E_r|``; flags, ``q`` and the loss interval are otherwise
unchanged.  The coded links are unchanged downstream: the decoders read this LLR tensor with the leaders' keys (scrambler stream 5,
information bits stream 8) and ``batch = G``.  What this models: R antennas, each estimated on its own.  Antenna correlation is not
this kernel's to model -- the estimators are per antenna, so a correlated channel has to be the channel the pilots saw --: it comes
from the simulator, ``ChannelSimConfig(antennas=(R, 1), rx_correlation=...)`` (chansim.py, "Kronecker frame groups"), whose groups are
these R frames and share one SNR, delay spread and Doppler.  With an ungrouped configuration the R frames are independent draws -- the
best case for the combiner -- each with its own conditions unless the caller pins them.  The link gives no array gain in the
estimator itself (no estimator here sees more than one antenna's pilots).  Diversity at the transmitter -- two antennas sending
one stream as Alamouti pairs in front of this combiner -- is "the transmit-diversity link" below (``tx_diversity=``).

The spatial-multiplexing link.  The receivers that have the antennas ``branches=`` models do not only combine: they separate two
spatial streams, and there an error in the estimate leaks one stream into the other, amplified by the conditioning of the channel.
``link_sm_host`` (float64), ``aft_link_sm_f32`` (csrc/k_linksm.hip, through ``hip_ops.LinkSmPlan``) and the ``streams=`` / ``detector=``
arguments of the accumulators and of the three sweeps of ``evaluation`` are linear detection of ``N = streams = 2`` transmit streams
on ``R = branches`` receive antennas, ``2 <= R <= 8``.  A batch of ``n`` frames with ``n % (N R) == 0`` is ``G = n / (N R)`` groups;
frame ``g N R + r N + s`` is the pair (antenna ``r``, stream ``s``) of group ``g``, ``H_{r,s}`` its true channel and ``E_{r,s}`` its estimate
(orthogonal pilots: each pair is estimated alone, at its own frame's SNR); frame ``(0, 0)`` is the group's LEADER::

    sent        stream s sends w_s, gi_s, gq_s, x_s exactly as the single link does, from stream 5 of the key of frame (0, s)
    received    y_r = H_{r,0} x_0 + H_{r,1} x_1 + sigma_r sqrt(-ln u1) exp(j 2 pi u2)     u1, u2 from streams 6, 7 of the key of frame (r, 0),
                                                                                           sigma_r that frame's; keys / sigma / rho of frames (r, 1)
                                                                                           beyond stream 5 of (0, 1) are not read
    weights     rho_r = float32(scale_{(r,0)} / scale_leader) as branch_weights forms them; scale = the leader's llr_scale, one float32 per group
    Gram        g00 = sum_r rho_r |E_r0|^2,  g11 = sum_r rho_r |E_r1|^2,  g01 = sum_r rho_r conj(E_r0) E_r1      increasing r, sums start at -0,
    matched     m_s = sum_r rho_r conj(E_rs) y_r                                                                   one fma per term as the combiner's
    regulariser reg float32 per group: 0 is zero forcing; float32(1 / scale) (formed in double, rounded once) is MMSE.  a00 = g00 + reg, a11 = g11 + reg
    detector    c_0 = a11 m_0 - g01 m_1            p_0 = g00 a11 - |g01|^2         (the adjugate: no division; p_s is det(A) less the MMSE bias,
                c_1 = a00 m_1 - conj(g01) m_0      p_1 = g11 a00 - |g01|^2          so comp >= beta_b p_s is the UNBIASED decision)
    hard        per stream the single link's decision, bit and symbol errors on (c_s, p_s) against (gi_s, gq_s)
    soft        eff_s = scale / a_other  (a11 for stream 0, a00 for stream 1; ONE correctly rounded float32 division; 0 where a_other <= 0)
                Lambda_j = eff_s Delta_j(c_s, p_s),  mu_k, Delta_j, the bit order and loss_f exactly the soft link's; pilots carry 0
    outputs     counts int [G, N, 2], loss [G, N, K], llr [G, N, S, T, m]: contiguous, so they read as G N frames with the keys of frames (0, s)

Why the soft rule holds: with noise variance ``1 / scale`` after the weights, the post-detection SINR of stream ``s`` is ``p_s scale /
a_other``, and that is the factor in front of ``|x^ - a_k|^2`` with ``x^ = c_s / p_s``.  The margin and the LLR reach follow the diversity
link's, with reaches that sum absolute values through the adjugate: ``reach(y_r) = |H_r0||x_0| + |H_r1||x_1| + |noise_r|``, ``reach(m_s) =
sum_r rho_r reach(y_r) |E_rs|``, ``G01 = sum_r rho_r |E_r0||E_r1|``, ``reach(c_0) = a11 reach(m_0) + G01 reach(m_1)`` and ``P_0 = g00 a11 +
G01^2`` (stream 1 symmetric); the margin is ``|comp - beta_b p_s| / (reach(c_s) + |beta_b| P_s)`` and ``q = eff_s A (A P_s + 2 reach(c_s))``.
The cancellation in ``p_s`` is inherent to separating two streams in float32 -- a nearly singular estimated channel has ``p_s`` far below
``P_s`` -- which is why the reaches are sums of absolute values and why the share of flagged decisions is larger than on the one-stream
links (tests/test_linksm.py holds the cap).  With an unheard second stream (``H_r1 = E_r1 = 0``) and ``reg scale = 1`` in powers of two,
stream 0 is the diversity link on the frames ``(r, 0)``.  Every rate of this link is per stream and symbol: the spectral efficiency is
N times it.  What this models: per-pair estimates and linear detection (zero forcing or MMSE; joint max-log detection is the next
section).  Antenna correlation, which decides how well two streams separate at all, comes from the simulator:
``ChannelSimConfig(antennas=(R, 2), rx_correlation=..., tx_correlation=...)`` makes these ``2 R`` frames one correlated group with
shared conditions (chansim.py, "Kronecker frame groups"); with an ungrouped configuration the pairs are independent draws with their
own conditions unless the caller pins them.  It does not model sphere or list detection, precoding, or ``N > 2``; ordered
successive cancellation behind this detector is "the successive-cancellation link" below (``detector="sic"``).  The same two transmit antennas sending ONE stream as Alamouti pairs are "the transmit-diversity link" below
(``tx_diversity=``).

The joint link.  A linear detector on a 2 x 2 Rayleigh channel has diversity order 1; a receiver that ships two-stream reception runs a
max-log joint demapper and gets order 2, and behind it an estimation error no longer leaks through an ill-conditioned inverse: it
enters as a mismatched metric.  ``link_joint_host`` (float64), ``aft_link_joint_f32`` (csrc/k_linksm.hip, through
``hip_ops.LinkJointPlan``) and ``detector="joint"`` (``JOINT_DETECTOR``; ``ALL_DETECTORS`` lists it after the linear ones) on the
accumulators and sweeps with ``streams=2`` are that demapper.  The layout, the keys, ``sent``, ``received``, ``weights`` and the eight sums
``m_0, m_1, g00, g11, g01`` are exactly the spatial-multiplexing link's: the same increasing ``r``, the same fused multiply-add per term,
sums that start at -0.  There is no regulariser and no division.  For stream ``e`` with the other stream ``o``, ``A = (L-1) d``, levels
``a_k`` and labels as on the soft link, and ``g_oe = g01`` for ``e = 1``, ``conj(g01)`` for ``e = 0``::

    candidates   x_e = a_ki + j a_kq over all M = 2^m words of stream e
    interference z(x_e) = m_o - g_oe x_e
    inner min    r(x_e) = min_k mu_k(Re z, g_oo) + min_k mu_k(Im z, g_oo)         mu_k(comp, p) = a_k (a_k p - 2 comp): the soft link's metric
    metric       f(x_e) = g_ee |x_e|^2 - 2 Re(conj(x_e) m_e) + r(x_e)            = min over x_o of sum_r rho_r |y_r - E_r0 x_0 - E_r1 x_1|^2, less a constant
    Delta_j      = min{f(x_e) : bit_j(word) = 1} - min{f(x_e) : bit_j(word) = 0}    bit order: the sent word's, I-axis bits first, MSB first
    LLR          Lambda_j = scale Delta_j        the leader's scale, one float32 per group; pilots carry 0
    hard         bit j is decided 1 iff Lambda_j < 0; bit errors against the sent word, a symbol error where any bit is wrong
    loss_f       the soft link's, on Lambda_j
    outputs      counts int [G, N, 2], loss [G, N, K], llr [G, N, S, T, m], as the spatial-multiplexing link's

Why: the weighted residual expands to ``const + sum_s (g_ss |x_s|^2 - 2 Re(conj(x_s) m_s)) + 2 Re(conj(x_0) g01 x_1)``, and for a fixed ``x_e``
the terms in ``x_o`` are ``g_oo |x_o|^2 - 2 Re(conj(x_o) z)``, the sum over the two axes of ``mu_k`` on a component of ``z``: the best ``x_o``
separates per axis.  So this is the exact max-log LLR of every bit of both streams in ``2 M`` candidate evaluations instead of ``M^2``.
The hard decision is the sign of the stream's own LLRs; without ties it is the joint ML pair, and the definition never has to say which
enumeration decides a stream.  What a float32 evaluation is compared through: ``Q = 2 A^2 (g00 + g11 + 2 G01) + 2 sqrt(2) A (reach(m_0) +
reach(m_1))`` with ``reach(m_s)`` and ``G01`` the spatial-multiplexing link's.  Every term of every ``f`` is bounded by its share of ``Q``:
``g_ee |x_e|^2 <= 2 A^2 g_ee`` and ``2 |x_e| |m_e| <= 2 sqrt(2) A reach(m_e)``; an axis of ``r`` is at most ``A^2 g_oo + 2 A |comp z|``, the two
together ``2 A^2 g_oo + 2 sqrt(2) A |z|``, and ``|z| <= reach(m_o) + sqrt(2) A G01`` turns that into ``2 A^2 g_oo + 2 sqrt(2) A reach(m_o) +
4 A^2 G01``; the shares add up to ``Q``, so ``|f| <= Q`` and ``|Delta_j| <= 2 Q``.  ``q = scale Q``; a data (element, stream, bit) is FLAGGED at
``tau`` when ``|Delta_j| <= tau Q``: an evaluation whose ``Delta`` is within ``tau Q`` can decide only flagged bits differently, so a
flagged bit moves a row's bit count by at most 1 and an (element, stream) with any flagged bit its symbol count by at most 1.  The
loss interval is the soft link's, at ``Lambda -+ e_lambda q``.  With an unheard second stream (``H_r1 = E_r1 = 0``) stream 1's ``Delta``
is exactly 0 and stream 0's LLRs are the diversity link's on the frames ``(r, 0)``.  What this models beyond the linear detectors: the
joint max-log demapper.  Antenna correlation comes from the simulator's grouped configurations, as for the linear detectors.  It does
not model sphere or list detection (nothing is pruned: every candidate is evaluated), iterative detection and decoding, or
``N > 2``; successive cancellation is the next section.

The successive-cancellation link.  The third textbook receiver for two streams (V-BLAST, MMSE-SIC) decides one stream with the linear
detector, rebuilds that stream's contribution from its own estimates, subtracts it and combines the other stream as a plain diversity
link.  It is the only receiver here in which an estimate error passes through a DECISION: a good estimate gives the second stream full
receive diversity at the linear detector's cost; a poor one fails twice, because a wrong first decision is subtracted with the wrong
gain.  ``link_sic_host`` (float64), ``aft_link_sic_f32`` (csrc/k_linksm.hip, through ``hip_ops.LinkSicPlan``) and ``detector="sic"``
(``SIC_DETECTOR``; ``LINK2_DETECTORS`` lists it after ``ALL_DETECTORS``) on the accumulators and sweeps with ``streams=2`` are that
receiver.  The layout, the keys, ``sent``, ``received``, ``weights``, the eight sums ``m_0, m_1, g00, g11, g01``, ``reg`` (float32 per
group, any value ``>= 0``; ``detector="sic"`` forms the MMSE one, ``detector_reg(scale, "mmse")``) and ``scale`` are exactly the
spatial-multiplexing link's: the same operands, the same increasing ``r``, the same fused multiply-add per term, sums that start at
-0.  Per data element::

    order      f = 1 iff g11 > g00, else f = 0 (a tie and NaN give 0); o = 1 - f.  This IS the order of the linear detector's post-detection
               SINRs p_s scale / a_other for every reg >= 0: p_0 a00 - p_1 a11 = (g00 - g11) det(A), det(A) = a00 a11 - |g01|^2 >= 0
    first      stream f: the linear detector's c_f, p_f, eff_f; its hard decision ki, kq, bit and symbol errors and LLRs
               eff_f Delta_j(c_f, p_f): exactly the spatial-multiplexing link's numbers for that (element, stream)
    decided    x^ = a_ki + j a_kq, a_k = d (2 k - (L - 1)), formed by the sent symbol's expression, so a correct decision is the very
               float32 symbol that was sent
    cancel     gx = g01 when o = 0, conj(g01) when o = 1  (= sum_r rho_r conj(E_ro) E_rf)
               c_o = m_o - gx x^,  p_o = g_oo.   Device: re = fma(-gx.re, x^.re, fma(gx.im, x^.im, m_o.re)),
               im = fma(-gx.re, x^.im, fma(-gx.im, x^.re, m_o.im))
    second     stream o: the DIVERSITY link's decision, errors, mu_k, Delta_j and Lambda_j = scale Delta_j(c_o, p_o), with the group's scale.
               No regulariser, no division.  After the weights the noise of c_o has variance p_o / scale, as on the diversity link
    outputs    counts int [G, N, 2], loss [G, N, K], llr [G, N, S, T, m]: indexed BY STREAM, not by detection order, so the decoders read
               them as they read the other two detectors'.  stats int32 [G, 3] per group: data elements with f = 1; data elements whose
               first decision is a symbol error; of those, elements where stream o also has a symbol error

Why the order needs no SINR: ``p_0 a00 - p_1 a11 = g00 a00 a11 - g11 a00 a11 + |g01|^2 (a11 - a00)`` and ``a11 - a00 = g11 - g00``, so the
difference is ``(g00 - g11) (a00 a11 - |g01|^2)``; the determinant is non-negative by Cauchy-Schwarz, hence ``SINR_1 > SINR_0`` exactly
when ``g11 > g00`` (tests/test_linksic.py compares the two).  The cancellation works on the sums themselves: the antennas are not
walked a second time and the second stage has no division.  Reaches: the first stage uses the spatial-multiplexing link's; the
second ``reach(c_o) = reach(m_o) + G01 |x^|`` and ``p_reach = p_o``, a sum of non-negative terms.  What a float32 evaluation is compared
through: a data element is ORDER-FLAGGED at ``tau`` when ``|g00 - g11| <= tau (g00 + g11)``, and DEPENDENT when it is order-flagged or
either axis of its first decision is flagged by the spatial-multiplexing link's margin.  At a dependent element the second stream's
outputs may differ freely -- its bit count by at most ``m``, its symbol count by at most 1, and its LLRs are only bounded, by
``2 q_dep`` with ``q_dep = scale A (A g_oo + 2 (reach(m_o) + sqrt(2) A G01))`` (every ``|x^| <= sqrt(2) A``) --; an order-flagged element
is dependent for BOTH streams (either may be the second one; the first-detected one is bounded by the linear detector's ``2 q``).
At every other element the second stream has its own flags and ``q = scale A (A p_o + 2 reach(c_o))``, as on the diversity link;
dependent bits of the second stream take ``-+ 2 q_dep`` in the loss interval.  ``link_sic_host(..., genie=True)`` is host only: it
cancels the SENT symbol of stream ``f`` instead of the decided one, the propagation-free bound.  With an unheard second stream
(``H_r1 = E_r1 = 0``) stream 0 is detected first everywhere and is the spatial-multiplexing link's stream 0 (the diversity link on the
frames ``(r, 0)`` for ``reg scale = 1`` in powers of two), and stream 1's LLRs are 0; with ``E_r1 = conj(E_r0)`` the Gram diagonal ties
and stream 0 is detected first everywhere.  ``sic_propagation()`` of a sweep reads the three integers as shares.  What this models:
symbol-level, ordered, hard-decision MMSE-SIC on per-pair estimates.  It does not model codeword-level or soft cancellation,
iterative detection and decoding, ``N > 2``, or HARQ (``HarqAccumulator`` gets no keyword, as today).

The codeword-cancellation link.  Symbol-level cancellation trusts hard symbol decisions, and most wrong first decisions repeat on the
other stream.  A two-codeword receiver cancels AFTER the decoder: a stream is subtracted only once its CRC has passed, so nothing wrong
is ever cancelled, and the estimate matters twice -- the receiver cancels ``E_ro x_o``, not ``H_ro x_o``, so the estimation error of the
cancelled stream stays behind as interference.  ``link_cancel_host`` (float64), ``cwsic_redetect``, ``link_cwsic_host``,
``aft_link_cancel_f32`` (csrc/k_linksm.hip, through ``hip_ops.LinkCancelPlan``), ``aft_link_ldpc_masked_f32`` (csrc/k_linkldpc.hip,
``hip_ops.LinkLdpcPlan(..., mask=)``) and ``detector="cwsic"`` (``CWSIC_DETECTOR``; ``CODED_DETECTORS`` lists it after
``LINK2_DETECTORS``) on ``LdpcBlockErrorAccumulator`` and ``evaluation.get_link_bler`` are that receiver.  Two streams on ``R = 2 .. 8``
antennas with the frame layout, keys, samples, weights and sums of the spatial-multiplexing link; an LDPC code on each stream; a
stream's transport block is the ``B`` blocks of its frame::

    first pass   MMSE detection of both streams: exactly link_sm_host / aft_link_sm_f32 with reg = float32(1 / scale); then LDPC decoding
                 of both: exactly link_ldpc_host / aft_link_ldpc_f32 on the 2 G frames with the keys of frames (0, s).
                 failed[g][s] = (the stream's block-error count != 0): an ideal CRC over all its blocks
    flags        redo[g][s] = failed[g][s] and not failed[g][1 - s]  (cwsic_redetect).  Both pass or both fail: nothing more happens
    cancel       for a stream s with redo, o = 1 - s, per data element:  c = m_s - g_so x_o,  g_so = g01 for s = 0 and conj(g01) for s = 1,
                 x_o the SENT symbol of stream o (an acknowledged codeword re-encodes to exactly the sent bits; filler bits are known
                 to the receiver);  p = g_ss.   Device: the successive-cancellation link's four fused multiply-adds (link_sic_cancel)
    re-detect    the diversity link's hard decision, errors, mu_k, Delta_j, Lambda_j = scale Delta_j and losses on (c, p) with the
                 group's scale: no regulariser, no division -- the successive-cancellation link's second stage with the sent symbol,
                 what link_sic_host(genie=True) computes for its second-detected stream.  A stream without redo has all-zero
                 outputs in this stage: LLRs, counts and losses
    second pass  LDPC decoding of the re-detected streams only (aft_link_ldpc_masked_f32 with the flags as its mask: a frame whose
                 word is 0 is not decoded and counts (0, 0, 0))
    final        a stream's bit and block errors are the second pass's where redo, the first pass's elsewhere; its iterations are
                 the sum of both passes

The residual ``(H_ro - E_ro) x_o`` that an imperfect estimate leaves in ``c`` is NOT modelled in the scale: the same simplification as the
successive-cancellation link's second stage, and the reason the share of re-detected streams that decode separates the estimators.
Blocks that a re-detected stream had acknowledged in the first pass are not kept separately: the unit is the stream, a known
simplification (a re-detected stream may lose a block it had; a per-block union would only lower the numbers).  Reaches for the
comparison of a float32 evaluation are the successive-cancellation link's second stage: ``reach(c) = reach(m_s) + G01 |x_o|`` and
``p_reach = g_ss``, with the sent symbol exact on both sides; flags, ``q`` and the loss interval as on the diversity link.  With an
unheard other stream (``H_ro = E_ro = 0``) a re-detected stream 0 is the diversity link on the frames ``(r, 0)``.  What this models:
hard, codeword-level, one-shot cancellation behind an ideal CRC.  It does not model a per-block union, soft or iterative cancellation,
HARQ, or ``N > 2``; ``"cwsic"`` is refused wherever no LDPC decoder runs (``LinkAccumulator``, ``RateAccumulator``,
``BlockErrorAccumulator``, ``HarqAccumulator``, ``streams=1``, ``tx_diversity=``, ``precoding_subband=``).

The transmit-diversity link.  The third standard two-antenna mode sends ONE stream from two transmit antennas as Alamouti pairs:
space-time block coding over adjacent symbols or space-frequency block coding over adjacent subcarriers, what cell-edge and control
transmissions of current OFDM systems run.  The pair is orthogonal only while the channel is equal across its two elements: time
pairing breaks with Doppler, frequency pairing with delay spread, and an estimation error shows up neither through an inverse nor
through a mismatched joint metric but as residual cross-talk between the two symbols of a pair.  ``link_alamouti_host`` (float64),
``alamouti_pairs``, ``alamouti_weights``, ``aft_link_alamouti_f32`` (csrc/k_linkalamouti.hip, through ``hip_ops.LinkAlamoutiPlan``)
and the ``tx_diversity=`` argument (one of ``PAIRINGS``) of the accumulators and of the three sweeps of ``evaluation`` are that link.
A batch of ``n`` frames with ``R = branches``, ``1 <= R <= 8`` and ``n % (2 R) == 0`` is ``G = n / (2 R)`` groups; frame
``g 2R + r 2 + s`` is the pair (receive antenna ``r``, transmit antenna ``s``) of group ``g`` -- the order of ``streams=2`` and of
``ChannelSimConfig(antennas=(R, 2))`` --, ``H_rs`` its true channel and ``E_rs`` its estimate; frame ``(0, 0)`` is the LEADER::

    lines      pairing "time": a line is a subcarrier s, its elements in increasing t;  pairing "frequency": a line is a symbol t, its
               elements in increasing s.  The DATA elements of a line in increasing order are d_0, d_1, ...; (d_2i, d_2i+1) is a pair
               (a, b), whether or not pilots lie between them; a line with an odd number of data elements leaves its last one LONE
    sent       every data element e sends w, gi, gq, x exactly as the single link does, from stream 5 of the LEADER's key at q_e = s T + t:
               one transmission per group, m data_elements bits (the code has rate 1)
    transmit   pair: antenna 0 sends x_a at a and -conj(x_b) at b; antenna 1 sends x_b at a and conj(x_a) at b.  Lone: antenna 0 sends x,
               antenna 1 nothing.  Each antenna sends at unit mean energy, as each stream of the spatial-multiplexing link does
    received   y_r[e] = H_r0[e] t0[e] + H_r1[e] t1[e] + sigma_r sqrt(-ln u1) exp(j 2 pi u2)      u1, u2 from streams 6, 7 of the key of frame
               (r, 0) at q_e, sigma_r that frame's; keys, sigma and rho of the frames (r, 1) are not read
    weights    rho_r = float32(scale_(r,0) / scale_leader) as branch_weights forms them over the 2 R frames; scale the leader's, one per group
    combiner   c_a = sum_r rho_r (conj(E_r0[a]) y_r[a] + E_r1[b] conj(y_r[b]))        p_a = sum_r rho_r (|E_r0[a]|^2 + |E_r1[b]|^2)
               c_b = sum_r rho_r (conj(E_r1[a]) y_r[a] - E_r0[b] conj(y_r[b]))        p_b = sum_r rho_r (|E_r1[a]|^2 + |E_r0[b]|^2)
               lone: c = sum_r rho_r conj(E_r0) y_r,  p = sum_r rho_r |E_r0|^2        (the diversity link's element on the frames (r, 0))
               increasing r; within r the term at a before the term at b; one fused multiply-add per term, as link_combine's
    hard/soft  the single link's decision, bit and symbol errors, mu_k, Delta_j, Lambda_j = scale Delta_j and loss_f on (c, p); pilots carry 0
    outputs    counts int [G, 2], loss [G, K], llr [G, S, T, m]: the diversity link's shapes, read by the decoders with the leaders' keys

Why the soft rule is the diversity link's: after the weights the noise of ``c`` has variance ``p / scale``, so ``scale`` stands in front
of ``p |x^ - a_k|^2`` exactly as there; there is no division and no regulariser.  Reaches, margins and ``q`` follow the diversity link's
with ``reach(y_r[e]) = |H_r0[e]||t0[e]| + |H_r1[e]||t1[e]| + |noise|`` and ``reach(c)`` the combiner's sum with every factor replaced
by its absolute value; ``p`` is a sum of non-negative terms, so ``p_reach = p``.  With an unheard second antenna (``H_r1 = E_r1 = 0``)
the first and the lone elements are the diversity link's on the frames ``(r, 0)``.  What this models: the linear Alamouti combiner,
which assumes the channel equal over a pair.  What is measured is the cross-talk left by channel variation inside a pair, by estimate
errors and by antenna correlation; correlation comes from the simulator, ``ChannelSimConfig(antennas=(R, 2), ...)``, whose groups are
these ``2 R`` frames.  The SNR is per transmit antenna, as on the spatial-multiplexing link: a comparison at equal total power
evaluates this link 3.01 dB lower.  It does not model joint detection of the two symbols of a pair, more than two transmit antennas,
or antenna selection; HARQ is not covered (``HarqAccumulator`` has no ``tx_diversity``).  The same two antennas co-phased by a
precoder the receiver feeds back are "the closed-loop link" below (``precoding_subband=``).

The closed-loop link.  The fourth standard two-antenna mode is the only one in which the channel estimate also acts at the
TRANSMITTER: in closed-loop rank-1 precoding the receiver picks a precoder from a small codebook using its estimates and reports the
index, a precoding matrix indicator (PMI), per subband; the two transmit antennas then send one stream co-phased by that precoder.  A
poor estimate hurts twice there: it picks the wrong precoder, and beamforming gain turns into loss; it then also mismatches the
combiner.  ``link_precoded_host`` (float64), ``precoding_subbands``, ``precoding_pmi_host``, ``precoding_weights``,
``aft_link_precoded_f32`` (csrc/k_linkprecode.hip, through ``hip_ops.LinkPrecodedPlan``) and the ``precoding_subband=`` argument of
the accumulators and of the three sweeps of ``evaluation`` are that link.  A batch of ``n`` frames with ``R = branches``,
``1 <= R <= 8`` and ``n % (2 R) == 0`` is ``G = n / (2 R)`` groups; frame ``g 2R + r 2 + s`` is the pair (receive antenna ``r``,
transmit antenna ``s``) of group ``g`` -- the order of ``streams=2``, of ``tx_diversity=`` and of ``ChannelSimConfig(antennas=(R, 2))``
--; frame ``(0, 0)`` is the LEADER.  ``B = precoding_subband`` with ``1 <= B <= S``::

    subbands   subband b = subcarriers b B .. min(S, (b+1) B) - 1, all T symbols; n_sub = ceil(S / B) (the last may be short; B = S is one
               wideband PMI).  n_sub <= AFT_LINK_MAX_SUBBANDS = 1024, else refused
    codebook   q_0 .. q_3 = 1, -1, j, -j; the precoder of index i is (1, q_i): antenna 0 sends x, antenna 1 sends q_i x.  Multiplying by q_i is
               a swap and negations: exact.  Each antenna sends at unit mean energy, as on the other two-antenna links
    selection  g_b = sum over the subband's S_b T elements (pilot positions included: the estimate is defined everywhere) and over r of
               rho_r conj(E_r0) E_r1;   v = (Re g_b, -Re g_b, -Im g_b, Im g_b) = Re(q_i g_b);   pmi_b = the LOWEST i that attains max v
               (g_b = 0 gives 0).  rho_r = the weights of the frames (r, 0), as alamouti_weights forms them (precoding_weights)
    sent       every data element sends w, gi, gq, x as the single link does, from stream 5 of the LEADER's key: one transmission per group
    received   y_r = H_r0 x + H_r1 (q x) + sigma_r sqrt(-ln u1) exp(j 2 pi u2)     q = q_pmi of the element's subband; u1, u2 from streams 6, 7 of the
               key of frame (r, 0), sigma_r that frame's; keys / sigma / rho of frames (r, 1) are not read
               (evaluated as H_r0 x + (q H_r1) x -- device: link_sample2 on (H_r0, q H_r1) with x1 = x -- so that the bits do not
               depend on a common turn of H_r1 and E_r1 by a power of j: q H_r1 is then the same number)
    effective  e_r = E_r0 + q E_r1       one rounding per component on the device
    combiner   c = sum_r rho_r y_r conj(e_r),  p = sum_r rho_r |e_r|^2     link_branch's chain per term, link_combine's fused multiply-add per sum,
               increasing r, starting value as link_mrc_kernel's
    hard/soft  the single link's decision, bit and symbol errors, mu_k, Delta_j, Lambda_j = scale Delta_j (leader's scale) and loss_f on (c, p);
               pilots carry 0
    outputs    counts int [G, 2], loss [G, K], llr [G, S, T, m] (the diversity link's shapes), and pmi int32 [G, n_sub]

Reaches for the comparison of a float32 evaluation follow the diversity link's: ``reach(y_r) = |H_r0||x| + |H_r1||x| + |noise|``,
``reach(e_r) = |E_r0| + |E_r1|``, ``reach(c) = sum rho reach(y_r) reach(e_r)`` and ``p_reach = sum rho reach(e_r)^2``: ``p`` is no longer
a sum of exact non-negative inputs, because ``e_r`` cancels.  The selection gets its own margin: with ``Gr_b = sum rho_r |E_r0||E_r1|``
over the subband, subband ``b`` is PMI-FLAGGED at ``tau_pmi`` when (largest ``v`` - second largest ``v``) ``<= tau_pmi Gr_b``; an
evaluation whose ``g_b`` is within ``tau_pmi Gr_b / 2`` per component can choose differently only at flagged subbands.  With an
unheard second antenna (``H_r1 = E_r1 = 0``) every PMI is 0 and the link is the diversity link on the frames ``(r, 0)``.  What this
models: instantaneous, error-free feedback of one PMI per subband, chosen from the same estimates the combiner uses, over all T symbols
(non-causal under Doppler); the total power is twice the single link's, so a comparison at equal total power evaluates this link
3.01 dB lower, as for Alamouti.  Open loop needs no feedback and has no array gain; closed loop has array gain exactly as far as the
estimate is good and the subband is narrower than the coherence bandwidth.  It does not model quantised CQI, feedback errors, rank
adaptation and rank-2 codebooks, more than two transmit antennas, or HARQ (``HarqAccumulator`` gets no keyword).

Delayed feedback.  How much of that gain survives when the precoder was chosen ``d`` slots ago, from an estimate of a channel that has
since moved: ``link_precoded_host(..., slots=K, delay=d)``, ``0 <= d < K`` (``precoding_pmi_host`` follows),
``aft_link_precoded_delayed_f32`` (the same kernel body, through ``hip_ops.LinkPrecodedPlan(..., slots=K, delay=d)``) and
``precoding_delay=d`` with ``slots=K`` on the accumulators and the sweeps.  The batch is whole SEQUENCES of K slots, a slot one group
of ``2 R`` frames -- the order of ``ChannelSimConfig(slots=K, antennas=(R, 2))``, whose slots are K consecutive stretches of one fading
process --: ``G = Q K`` input groups, input group ``seq K + k`` slot ``k`` of sequence ``seq``::

    warm-up    slots k < d of a sequence are not transmitted and produce no output
    selection  slot k >= d is transmitted with, per subband, the PMI selected from the estimates and rho of slot k - d of the same sequence:
               the selection above, operation for operation, on the FEEDBACK group
    the rest   the received samples, e_r = E_r0 + q E_r1, the combiner, the decision, the LLRs and the losses use the TRANSMIT slot's own
               H, E, keys, sigma, rho and scale, exactly as above
    outputs    compact: output group o = seq (K - d) + (k - d); counts, loss, llr and pmi have Q (K - d) rows; pmi is the APPLIED index

With ``d = 0`` every slot is its own feedback slot: the link above, bit for bit, whatever K.  The receiver still combines with the
effective estimate of the precoder that was applied (it knows what it fed back), so a stale PMI costs array gain, not a mismatch.
``frames`` and every rate count transmitted groups only.  Not modelled: quantised CQI, feedback errors, rank adaptation, more than two
transmit antennas, HARQ over precoded transmissions.

The coded link.  The rate says how much information the LLRs carry; a link-level user wants the same with a decoder in the loop: the
block-error rate of coded blocks and the throughput that follows from it.  ``CodeConfig``, ``link_encode_host`` / ``link_decode_host``
(integer NumPy), ``aft_link_decode_f32`` (csrc/k_linkcode.hip, through ``hip_ops.LinkDecodePlan``), ``BlockErrorAccumulator`` and
``evaluation.get_link_bler`` are to it what the names above are to the bit errors.  The link is unchanged -- a frame still sends the
words ``w`` of stream 5 -- and the code rides on it through a scrambler both ends know::

    code         rate 1/2, constraint length 7, zero-terminated.  Inputs u_0 .. u_{K-1}; u_t = 0 for t < 0 and K <= t < K + 6.
                 For t = 0 .. K + 5:   A_t = u_t ^ u_{t-2} ^ u_{t-3} ^ u_{t-5} ^ u_{t-6}       (133 octal)
                                       B_t = u_t ^ u_{t-1} ^ u_{t-2} ^ u_{t-3} ^ u_{t-6}       (171 octal)
                 u = 1,0,0,0,0,0,0 gives A = 1,0,1,1,0,1,1 and B = 1,1,1,1,0,0,1: weight 10
    puncturing   by t mod P, the 802.11 patterns: rate 1/2 (P = 1) keeps A B; 2/3 (P = 2) keeps A0 B0 A1; 3/4 (P = 3) keeps A0 B0 A1 B2.
                 The kept bits in step-major order, A before B, are the n coded bits of a block
                 (K = 512: n = 1036 at rate 1/2 and 691 at 3/4; K = 1024: n = 1374 at 3/4)
    blocks       N = m data_elements bits per frame, B = N // n blocks (B = 0 is refused), U = B n used bits.  Data-bit index j is
                 bit k = j % m -- the last axis of the LLR tensor, bit (w >> (m-1-k)) & 1 of the sent word -- of the (j // m)-th grid
                 element that is no pilot, in row-major order.  Bits j >= U are filler: sent as the link sends them, ignored by the
                 decoder.  LLRs at pilot positions are never read
    interleaver  coded bit i of block b, p = b n + i, sits at j = (p A) mod U with gcd(A, U) = 1.  The default stride A is the smallest
                 integer >= max(1, floor(0.3819660112501051 U)) coprime to U (a golden-section stride); U >= 10, so 1 <= A < U
    information  u[b][t] = word(kf, stream 8, b K + t) >> 63            (B K <= 2^31: the hash's index is 32 bits, the counts are int32)
    input        scrambler s_p = w_j ^ c_p with c_p the coded bit;  lambda_p = (1 - 2 s_p) llr_j;
                 z_p = clamp(rint(float32(lambda_p qgain)), -127, 127): ONE float32 product, to nearest with ties to even, NaN gives 0
                 (qgain = 8: steps of 1/8, clipped at +-15.875)
    Viterbi      state sigma = sum_{i=1..6} u_{t-i} 2^(6-i), successor (sigma >> 1) | (u_t << 5).  int32 metrics, M[0] = 0 and
                 -2^30 elsewhere.  A branch gains the sum over its kept outputs of (1 - 2 out) z; a punctured output gives nothing.
                 State n has predecessors r0 = (n & 31) << 1 and r1 = r0 | 1 with input n >> 5; the survivor is the larger sum and A
                 TIE TAKES r0: the decision bit is 1 only when r1 is strictly larger.  Traceback from state 0 after K + 6 steps:
                 u^_t = n >> 5, previous state ((n & 31) << 1) | decision.  K <= 4090: 4096 steps of at most 254 each overflow nothing
    result       (information-bit errors over the B K bits, blocks with any error) per frame

Everything after the quantiser is integer, so the host and the device agree bit for bit on the same float32 LLRs: no tolerance.  The
path a tie-breaking Viterbi returns is, of all paths of the largest metric, the one whose inputs read from the last to the first are
smallest (each merge prefers the older input 0), which is what tests/test_linkcode.py's brute force over all 2^K inputs compares.
The LDPC-coded link.  Data channels of current OFDM systems run LDPC codes, and an iterative decoder reacts to LLR quality (a cliff,
and a sensitivity to mis-scaled LLRs) unlike a Viterbi decoder.  ``LdpcConfig``, ``ldpc_base``, ``ldpc_encode``,
``link_ldpc_encode_host`` / ``ldpc_decode_host`` / ``link_ldpc_host`` (integer NumPy), ``aft_link_ldpc_f32`` (csrc/k_linkldpc.hip,
through ``hip_ops.LinkLdpcPlan``), ``LdpcBlockErrorAccumulator`` and ``evaluation.get_link_bler`` are the same surface for a
quasi-cyclic LDPC code with a layered offset min-sum decoder.  Position on the link, hash streams, scrambler and quantiser are the
convolutional code's::

    code         quasi-cyclic, lifting Z = 64.  Base matrix of mb rows and nb columns, 3 <= mb <= 16, mb < nb <= 32, kb = nb - mb;
                 n = 64 nb coded and K = 64 kb information bits.  An entry is -1 (no block) or a shift s in 0 .. 63: block (i, j)
                 with shift s has, in its row r, its one at column (r + s) mod 64 -- check 64 i + r contains variable
                 64 j + ((r + s) mod 64)
    parity part  columns kb .. nb-1, fixed by structure, mid = mb // 2: column kb has shift 1 in rows 0 and mb-1 and shift 0 in row
                 mid; column kb + 1 + i (i = 0 .. mb-2) has shift 0 in rows i and i + 1
    information  an int32 table [mb][kb]: every entry in -1 .. 63, every column with at least one entry, at most 160 entries
    part         (AFT_LINK_LDPC_MAX_EDGES) over the whole base matrix, parity part included.  The default is ldpc_base(mb, nb, seed):
                 offsets o = (0, 1, mb//2 - 1) if mb >= 8 else (0, 1, 2); for j = 0 .. kb-1 and t = 0, 1, 2 in that order the row is
                 r = (j + o[t]) mod mb, h = splitmix64(seed ^ (9 << 32 | 4 j + t)) >> 58 (stream 9), and the shift is (h + c) mod 64
                 for the smallest c in 0 .. 63 that closes no 4-cycle with what is already placed (the parity columns, information
                 columns < j, column j's earlier t): v is refused when for an already-placed row r2 of column j and another column
                 b with entries in both r and r2, (v - S[r2][j]) mod 64 == (S[r][b] - S[r2][b]) mod 64.  No c: ValueError
    rates        "1/2" = (12, 24), "2/3" = (8, 24), "3/4" = (6, 24): n = 1536; or any (mb, nb)
    encoding     u_j the 64 bits of block column j, rot(x, s)[r] = x[(r + s) mod 64]:  lam_i = XOR_j rot(u_j, S[i][j]) over the row's
                 information blocks;  p_0 = XOR_i lam_i;  p_1 = lam_0 ^ rot(p_0, 1);  p_{i+1} = lam_i ^ p_i ^ (p_0 if i == mid else 0)
                 for i = 1 .. mb-2;  the codeword is u | p_0 | .. | p_{mb-1}
    position     B = N // n blocks (B = 0 is refused), U = B n, interleaver j = (b n + i) stride mod U with the same default stride,
                 u[b][t] = word(kf, stream 8, b K + t) >> 63, scrambler s_p = w_j ^ c_p,
                 z_p = clamp(rint(float32((1 - 2 s_p) llr_j qgain)), -127, 127), NaN gives 0
    decoder      layered offset min-sum, integer.  Posterior L_v = z_v, messages R = 0; offset beta in 0 .. 127 (default 4),
                 max_iters I in 1 .. 255 (default 20).  For iteration 1 .. I and layer i = 0 .. mb-1 -- its edges e the nonzero base
                 columns in increasing order, parity included -- each of the layer's 64 rows on its own:
                   Q_e = L_v(e) - R_e (all Q of a layer before any update);  neg_e = Q_e < 0;  tot = XOR_e neg_e;
                   m1 = min_e |Q_e| at the lowest e that attains it, a;  m2 = min_{e != a} |Q_e|;
                   mag_e = min(max((m2 if e == a else m1) - beta, 0), 127);  R_e = -mag_e if tot ^ neg_e else +mag_e;
                   L_v(e) = clamp(Q_e + R_e, -8191, 8191)
                 After each whole iteration x_v = [L_v < 0]; the decoder stops when all 64 mb checks hold, or after I iterations.
                 The decoded bits are x_0 .. x_{K-1}
    result       (information-bit errors, blocks with any error, iterations run summed over the B blocks) per frame

Messages fit int8 and posteriors int16.  Rows of one layer share no variable (a block column holds at most one block per layer, and
a circulant is a permutation), so the order of a layer's rows does not matter: tests/test_linkldpc.py decodes row by row over the
expanded matrix and compares for equality.

The HARQ link.  Every coded number above is a single-shot block-error rate at a fixed code rate.  A data channel runs hybrid ARQ: a
block that fails is sent again, and the receiver adds the new soft bits to the old ones and decodes again, so an estimator's gain
shows as fewer retransmissions and as throughput at SNRs where the single-shot rate is 1 for every estimator.  ``HarqConfig``,
``link_harq_host`` (integer NumPy), ``aft_link_harq_f32`` (csrc/k_linkharq.hip, through ``hip_ops.LinkHarqPlan``), ``HarqAccumulator``
and ``evaluation.get_link_harq`` are that surface::

    mother code   an LdpcConfig ``code``: base matrix mb x nb, kb = nb - mb, n = 64 nb, K = 64 kb; encoder and decoder unchanged.  It
                  must itself be valid on the link (N >= n); its own stride and blocks are not used
    rate matching tx_cols = C with kb < C <= nb: a round sends E = 64 C coded bits per block.  rounds = Q in 1 .. 4
                  (AFT_LINK_HARQ_MAX_ROUNDS).  starts = (s_0 .. s_{Q-1}), each in 0 .. nb-1: the block column where a round's window
                  begins.  Transmitted bit e = 0 .. E-1 of round t is codeword bit v_t(e) = 64 ((s_t + e // 64) mod nb) + e % 64: a
                  circular buffer in whole block columns.  mode "ir" (incremental redundancy) gives s_t = (t C) mod nb, each round
                  continuing where the last ended; mode "chase" gives s_t = 0
    position      N = m data_elements bits per frame, B = N // E blocks (B K <= 2^31), U = B E.  Transmitted bit e of block b sits at
                  data-bit index j = ((b E + e) A) mod U, A the golden-section default_stride(U) or a given stride coprime to U; j maps
                  to a grid element and a bit of its word exactly as on the coded links; filler and pilots are never read
    groups        the LLR frames h Q .. h Q + Q - 1 (keys k_0 .. k_{Q-1}) are rounds 0 .. Q-1 of group h, k_0 its LEADER.
                  u[b][i] = word(k_0, stream 8, b K + i) >> 63 and c = ldpc_encode(u).  Round t uses its OWN frame's sent words, w
                  from stream 5 of k_t: scrambler s = w_j ^ c[v_t(e)], z_{t,b,e} = quantise((1 - 2 s) llr_t[j]) with the code's qgain
    soft buffer   Z_t[b][v] = the sum over t' <= t and over e with v_{t'}(e) = v of z_{t',b,e}: an integer, |Z| <= 127 Q, 0 where
                  nothing has been sent yet
    attempts      after round t every block not yet acknowledged is decoded from scratch, L = Z_t and R = 0, with the offset,
                  max_iters, layer order, clamps and syndrome stop rule of the LDPC-coded link.  A block is ACKNOWLEDGED iff its
                  decoded information bits equal u -- an ideal CRC: a wrong codeword that satisfies the syndrome is not acknowledged.
                  An acknowledged block runs no further attempt; later rounds' LLRs at its positions influence nothing
    counts        int [groups][7] (AFT_LINK_HARQ_COUNTS): columns 0 .. 3 the blocks first acknowledged after round t (0 for t >= Q),
                  4 the information-bit errors of the blocks never acknowledged, from their last attempt, 5 the blocks never
                  acknowledged, 6 the iterations summed over all attempts run
    bits          uint8 [groups, B, K]: each block's decoded information bits from the last attempt it ran

With Q = 1, C = nb, s_0 = 0 and the same stride this is the LDPC-coded link: column 0 is B less its block errors, columns 4, 5 and 6
its bit errors, block errors and iterations, and the bits are equal bit for bit.

The decision-directed observation.  Every estimator sees the pilots only; a receiver that has demodulated a frame can re-estimate the
channel from its own decisions.  On the diversity link's groups (R frames, one transmission, the leader's key), with that link's y_r,
c and p::

    decision      (ki, kq), per axis the number of inner boundaries beta_b p at or below the component of c: the diversity link's own
    x^            d (2 ki - (L - 1)) + j d (2 kq - (L - 1)); with source="sent" the sent x (the genie bound)
    z_r[s, t]     y_r conj(x^) / |x^|^2 = H_r + (H_r (x - x^) + noise_r) conj(x^) / |x^|^2 at a data element: the channel plus noise of
                  variance sigma_r^2 / |x^|^2 where the decision is right; frame r's own noisy pilot at a pilot position
    decisions     uint8 [G, S, T], ki | kq << 4, and 255 at the pilots
    symbol_errors int64 [G], the data elements whose (ki, kq) differ from the sent level indices

``link_observe_host`` is the float64 twin, ``aft_link_observe_f32`` (csrc/k_linkobserve.hip, ``hip_ops.LinkObservePlan``) the device's
one launch per batch.  ``data_noise_scale(m)``, the constellation's mean of 1 / |a|^2, is the factor the full-grid smoother
(``lmmse.lmmse_grid_host``) puts on the noise variance; ``DataAidedRefiner`` is observe-then-smooth, iterated, and the ``refine=``
keyword of the sweeps in ``evaluation`` runs it between the estimator and the accumulator.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _abi
from .chansim import (STREAM_CODE_BITS, STREAM_DATA_BITS, STREAM_DATA_NOISE_ANGLE, STREAM_DATA_NOISE_RADIUS, STREAM_LDPC_SHIFTS,
                      ChannelSimConfig, frame_keys, words)
from .synth import _splitmix64

BITS_PER_SYMBOL = (2, 4, 6, 8)
_POPCOUNT = np.array([bin(i).count("1") for i in range(16)], dtype=np.int64)


@dataclass(frozen=True)
class LinkConfig:
    """The link a frame's errors are counted on: the simulator's grid and pilot positions, and the modulation order."""
    sim: ChannelSimConfig = field(default_factory=ChannelSimConfig)
    bits_per_symbol: int = 4

    def __post_init__(self) -> None:
        if not isinstance(self.sim, ChannelSimConfig):
            raise ValueError(f"LinkConfig needs a chansim.ChannelSimConfig (got {type(self.sim).__name__})")
        m = self.bits_per_symbol
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or int(m) not in BITS_PER_SYMBOL:
            raise ValueError(f"bits_per_symbol = {m!r}: square QAM with one of {BITS_PER_SYMBOL} bits per symbol")
        object.__setattr__(self, "bits_per_symbol", int(m))
        S, T = self.sim.ofdm
        if S * T > 1 << 31:
            raise ValueError(f"ofdm grid {S} x {T}: the element index of the hash is 32 bits, at most 2^31 elements")

    @property
    def levels(self) -> int:
        return 1 << (self.bits_per_symbol // 2)

    @property
    def d(self) -> float:
        """Half the distance between neighbouring levels, for unit mean symbol energy."""
        return float(np.sqrt(3.0 / (2.0 * (self.levels ** 2 - 1.0))))

    @property
    def data_mask(self) -> np.ndarray:
        """bool ``[S, T]``: True where the grid carries data (everywhere but ``pilot_scs x pilot_symbols``)."""
        mask = np.ones(self.sim.ofdm, dtype=bool)
        mask[np.asarray(self.sim.pilot_scs)[:, None], np.asarray(self.sim.pilot_symbols)[None, :]] = False
        return mask

    @property
    def data_elements(self) -> int:
        return self.sim.ofdm[0] * self.sim.ofdm[1] - self.sim.pilot[0] * self.sim.pilot[1]

    @property
    def bits_per_frame(self) -> int:
        return self.bits_per_symbol * self.data_elements

    def to_struct(self) -> "_abi.AftLink":
        p = self.sim.fill_grid(_abi.AftLink())
        p.bits_per_symbol = self.bits_per_symbol
        return p


def noise_sigma(snr_db) -> np.ndarray:
    """``float32(10^(-snr_db / 20))``: formed in double, rounded once."""
    return (10.0 ** (-np.asarray(snr_db, dtype=np.float64) / 20.0)).astype(np.float32)


def gray_level(g) -> np.ndarray:
    """The level index ``k`` of a Gray code of at most four bits: ``k ^ (k >> 1) = g``."""
    g = np.asarray(g, dtype=np.int64)
    g = g ^ (g >> 1)
    return g ^ (g >> 2)


def constellation(bits_per_symbol: int) -> np.ndarray:
    """complex128 ``[2^m]``: the symbol every m-bit word ``w`` is sent as."""
    cfg = LinkConfig(bits_per_symbol=bits_per_symbol)
    m, L = cfg.bits_per_symbol, cfg.levels
    w = np.arange(1 << m)
    ki, kq = gray_level(w >> (m // 2)), gray_level(w & (L - 1))
    return cfg.d * ((2 * ki - (L - 1)) + 1j * (2 * kq - (L - 1)))


def _uniform(keys: np.ndarray, stream: int, q: np.ndarray) -> np.ndarray:
    return ((words(keys, stream, q) >> np.uint64(41)).astype(np.float64) + 0.5) * 2.0 ** -23


def _checked(cfg: LinkConfig, keys, ideal, est, sigma):
    """The operands of a definition, checked: ``(keys uint64 [n], H, E complex128 [n, S, T], sigma float64 [n])``."""
    keys = np.ascontiguousarray(keys)
    if keys.dtype == np.int64:
        keys = keys.view(np.uint64)
    if keys.dtype != np.uint64 or keys.ndim != 1:
        raise ValueError("keys must be a vector of 64-bit words (uint64, or int64 taken bit for bit)")
    n, (S, T) = len(keys), cfg.sim.ofdm
    H, E = np.asarray(ideal).astype(np.complex128), np.asarray(est).astype(np.complex128)
    if H.shape != (n, S, T) or E.shape != (n, S, T):
        raise ValueError(f"Expected ideal and est of shape ({n}, {S}, {T}), got {H.shape} and {E.shape}")
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if sigma.shape != (n,):
        raise ValueError(f"sigma must hold one value per frame ({n}), got {sigma.size}")
    return keys, H, E, sigma


def _sent(cfg: LinkConfig, keys: np.ndarray):
    """The sent word of every element of the transmissions with ``keys``: the Gray codes ``gi`` / ``gq`` and the symbol ``x``."""
    (S, T), m, L, d = cfg.sim.ofdm, cfg.bits_per_symbol, cfg.levels, cfg.d
    q = np.arange(S * T, dtype=np.uint64).reshape(1, S, T)
    w = (words(keys[:, None, None], STREAM_DATA_BITS, q) >> np.uint64(64 - m)).astype(np.int64)
    gi, gq = w >> (m // 2), w & (L - 1)
    return gi, gq, d * ((2 * gray_level(gi) - (L - 1)) + 1j * (2 * gray_level(gq) - (L - 1)))


def _noise(cfg: LinkConfig, keys: np.ndarray, sigma) -> np.ndarray:
    """The data noise of the frames with ``keys``: ``sigma sqrt(-ln u1) exp(j 2 pi u2)``, complex128 ``[n, S, T]``."""
    S, T = cfg.sim.ofdm
    q = np.arange(S * T, dtype=np.uint64).reshape(1, S, T)
    kk = keys[:, None, None]
    u1, u2 = _uniform(kk, STREAM_DATA_NOISE_RADIUS, q), _uniform(kk, STREAM_DATA_NOISE_ANGLE, q)
    return sigma[:, None, None] * np.sqrt(-np.log(u1)) * np.exp(2j * np.pi * u2)


def _branch(cfg: LinkConfig, keys: np.ndarray, H, E, sigma, x):
    """One receive branch per key: ``c = y conj(E)`` with ``y = H x`` plus the noise of the branch's own key, ``p = |E|^2`` and the
    reach ``(|H||x| + |noise|) |E|`` of a component of ``c``."""
    noise = _noise(cfg, keys, sigma)
    c = (H * x + noise) * E.conj()
    p = E.real ** 2 + E.imag ** 2
    reach = (np.abs(H) * np.abs(x) + np.abs(noise)) * np.abs(E)
    return c, p, reach


def _front(cfg: LinkConfig, keys, ideal, est, sigma):
    """What the hard and the soft definition share, in float64: the checked operands and, per element, the sent Gray codes ``gi`` / ``gq``,
    ``c = y conj(E)``, ``p = |E|^2`` and the reach ``(|H||x| + |noise|) |E|`` of a component of ``c``."""
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    gi, gq, x = _sent(cfg, keys)
    return (gi, gq, *_branch(cfg, keys, H, E, sigma, x))


def link_errors_host(cfg: LinkConfig, keys, ideal, est, sigma, tau: Optional[float] = None):
    """The definition in float64 on the given arrays: ``keys`` uint64 ``[n]`` (an int64 array is taken bit for bit), ``ideal`` / ``est``
    complex ``[n, S, T]``, ``sigma`` ``[n]`` -> ``counts`` int64 ``[n, 2]`` = (bit errors, symbol errors) per frame.  With ``tau``:
    ``(counts, errors, flags)``, ``errors`` int64 ``[n, S, T]`` the wrong bits of each element (0 at the pilots) and ``flags`` bool
    ``[n, S, T, 2]`` the flagged (element, axis) pairs at ``tau`` (module docstring; False at the pilots).  Needs no library."""
    return _hard(cfg, *_front(cfg, keys, ideal, est, sigma), tau)


def _hard(cfg: LinkConfig, gi, gq, c, p, reach, tau, p_reach=None):
    """The hard decision and the margins on ``c`` and ``p``: what ``link_errors_host`` returns.  ``p_reach``: the reach of ``p`` where it
    is not ``p`` itself (the spatial-multiplexing link, whose ``p`` is a difference)."""
    p_reach = p if p_reach is None else p_reach
    (n, S, T), L, d = c.shape, cfg.levels, cfg.d
    mask = cfg.data_mask[None]
    if tau is not None:
        flags = np.zeros((n, S, T, 2), dtype=bool)
    wrong = np.zeros((n, S, T), dtype=np.int64)
    for axis, (comp, sent) in enumerate(((c.real, gi), (c.imag, gq))):
        level = np.zeros((n, S, T), dtype=np.int64)
        for b in range(1, L):
            beta = 2.0 * d * (b - L / 2)
            level += comp >= beta * p
            if tau is not None:
                den = reach + abs(beta) * p_reach
                margin = np.divide(np.abs(comp - beta * p), den, out=np.zeros_like(den), where=den > 0)
                flags[..., axis] |= margin <= tau
        wrong += _POPCOUNT[sent ^ level ^ (level >> 1)]
    wrong *= mask
    counts = np.stack([wrong.sum(axis=(1, 2)), (wrong > 0).sum(axis=(1, 2))], axis=1).astype(np.int64)
    if tau is None:
        return counts
    flags &= mask[..., None]
    return counts, wrong, flags


DEFAULT_FACTORS = tuple(2.0 ** -k for k in range(8))        # 1, 1/2, ..., 1/128: the grid the GMI's supremum over the LLR scale is taken on
MAX_FACTORS = 8


def llr_scale(snr_db, err_var=0.0) -> np.ndarray:
    """``float32(1 / (10^(-snr_db / 10) + err_var))``: one over the noise variance plus the estimate's error variance, formed in double
    and rounded once."""
    return (1.0 / (10.0 ** (-np.asarray(snr_db, dtype=np.float64) / 10.0) + float(err_var))).astype(np.float32)


def _factors(factors) -> np.ndarray:
    f = np.asarray(factors, dtype=np.float32).reshape(-1)
    if not 1 <= f.size <= MAX_FACTORS:
        raise ValueError(f"between 1 and {MAX_FACTORS} factors, got {f.size}")
    return f


def link_llrs_host(cfg: LinkConfig, keys, ideal, est, sigma, scale, factors=(1.0,), e_lambda: Optional[float] = None):
    """The soft definition (module docstring) in float64: operands as ``link_errors_host``'s, ``scale`` ``[n]`` and ``factors`` ``[K]``
    taken as the float32 numbers they are -> ``(loss float64 [n, K], llr float64 [n, S, T, m])``, the LLRs 0 at the pilots.  With
    ``e_lambda``: ``(loss, llr, loss_lo, loss_hi, q)``, ``q [n, S, T, m] = scale A (A p + 2 R)`` (0 at the pilots) and ``loss_lo`` /
    ``loss_hi`` the losses at ``Lambda -+ e_lambda q``, every bit moved towards / away from the sent bit.  Needs no library."""
    return _soft(cfg, *_front(cfg, keys, ideal, est, sigma), scale, factors, e_lambda)


def _gray_split(metric: np.ndarray, half: int) -> list:
    """Per bit ``j`` of an axis's Gray label (MSB first) the minimum of ``metric [..., L]`` over the levels whose bit is 1 less the
    minimum over those whose bit is 0: ``half`` arrays."""
    k = np.arange(metric.shape[-1])
    ones = [((((k ^ (k >> 1)) >> (half - 1 - j)) & 1).astype(bool)) for j in range(half)]
    return [metric[..., one].min(axis=-1) - metric[..., ~one].min(axis=-1) for one in ones]


def _sent_signs(gi: np.ndarray, gq: np.ndarray, half: int) -> np.ndarray:
    """``1 - 2 b_j`` of the sent Gray codes ``[...]`` -> float64 ``[..., m]``, I-axis bits first, MSB first."""
    sign = np.empty((*gi.shape, 2 * half))
    for axis, sent in enumerate((gi, gq)):
        for j in range(half):
            sign[..., axis * half + j] = 1 - 2 * ((sent >> (half - 1 - j)) & 1)
    return sign


def _losses_at(sign: np.ndarray, mask: np.ndarray, factors: np.ndarray):
    """``lam [..., S, T, m]`` -> the losses ``[..., K]`` of the LLRs ``lam`` against the sent bits at the factors, in bits."""
    def losses(lam):
        z = -(sign * lam)
        return np.stack([(np.logaddexp(0.0, f * z) * mask).sum(axis=(-3, -2, -1)) for f in factors], axis=-1) / np.log(2.0)
    return losses


def _soft(cfg: LinkConfig, gi, gq, c, p, reach, scale, factors, e_lambda, p_reach=None):
    """The LLRs and the losses on ``c`` and ``p``: what ``link_llrs_host`` returns.  ``scale`` float64 ``[n, S, T]`` is taken per element
    as it is (the spatial-multiplexing link's ``eff``, with ``p_reach`` the reach of its ``p``)."""
    (n, S, T), m, L, d = c.shape, cfg.bits_per_symbol, cfg.levels, cfg.d
    half = m // 2
    if np.ndim(scale) == 3:
        scale = np.asarray(scale, dtype=np.float64).reshape(n, S * T)
    else:
        scale = np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(-1)
        if scale.shape != (n,):
            raise ValueError(f"scale must hold one value per frame ({n}), got {scale.size}")
        scale = scale[:, None]
    scale = np.broadcast_to(scale, (n, S * T)).reshape(n, S, T)
    p_reach = p if p_reach is None else p_reach
    factors = _factors(factors).astype(np.float64)
    a = d * (2 * np.arange(L) - (L - 1))
    mask = cfg.data_mask[None, :, :, None]
    llr = np.empty((n, S, T, m))
    for axis, comp in enumerate((c.real, c.imag)):
        mu = a * (a * p[..., None] - 2.0 * comp[..., None])                      # [n, S, T, L]
        for j, delta in enumerate(_gray_split(mu, half)):
            llr[..., axis * half + j] = delta
    llr *= scale[..., None] * mask
    sign = _sent_signs(gi, gq, half)                           # 1 - 2 b_j
    losses = _losses_at(sign, mask, factors)
    loss = losses(llr)
    if e_lambda is None:
        return loss, llr
    A = (L - 1) * d
    q = np.broadcast_to((scale * A * (A * p_reach + 2.0 * reach))[..., None] * mask, llr.shape).copy()
    return loss, llr, losses(llr + sign * (e_lambda * q)), losses(llr - sign * (e_lambda * q)), q


MAX_BRANCHES = _abi.AFT_LINK_MAX_BRANCHES


def _branches(branches) -> int:
    if isinstance(branches, bool) or not isinstance(branches, (int, np.integer)) or not 1 <= int(branches) <= MAX_BRANCHES:
        raise ValueError(f"branches = {branches!r}: an integer in 1 .. {MAX_BRANCHES}")
    return int(branches)


def _grouped(n: int, branches: int, streams: int = 1) -> int:
    if streams > 1 and n % (branches * streams):
        raise ValueError(f"a batch of {n} frames is not a multiple of branches * streams = {branches} * {streams}")
    if n % branches:
        raise ValueError(f"a batch of {n} frames is not a multiple of branches = {branches}")
    return n // (branches * streams)


def _weights(scale: np.ndarray, branches: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(rho float32 [n], the leaders' scale float32 [G])`` of the frames' float32 LLR scales ``[n]``."""
    s = np.asarray(scale, dtype=np.float32).reshape(_grouped(np.size(scale), branches), branches)
    rho = (s.astype(np.float64) / s[:, :1].astype(np.float64)).astype(np.float32)
    return rho.reshape(-1), np.ascontiguousarray(s[:, 0])


def branch_weights(snr_db, err_var: float = 0.0, branches: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """The combiner's weights for frames at ``snr_db`` ``[n]`` (module docstring, "the diversity link"): ``(rho float32 [n], scale
    float32 [G])``, ``rho_r = float32(scale_r / scale_leader)`` and ``scale`` the leaders' ``llr_scale(snr_db, err_var)``."""
    return _weights(llr_scale(np.asarray(snr_db, dtype=np.float64).reshape(-1), err_var), _branches(branches))


def link_mrc_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, scale, branches, factors=(1.0,), tau: Optional[float] = None,
                  e_lambda: Optional[float] = None):
    """The diversity link (module docstring) in float64: ``keys`` / ``ideal`` / ``est`` / ``sigma`` as ``link_errors_host``'s for the
    ``n`` frames, ``rho`` ``[n]`` and ``scale`` ``[G]`` taken as the float32 numbers they are (``branch_weights``), ``G = n / branches``
    -> ``(counts int64 [G, 2], loss float64 [G, K], llr float64 [G, S, T, m])``.  With ``tau`` the wrong-bit map ``[G, S, T]`` and the
    flags ``[G, S, T, 2]`` follow, with ``e_lambda`` then ``loss_lo``, ``loss_hi`` and ``q``: what ``link_errors_host`` and
    ``link_llrs_host`` return, on the combined ``c``, ``p`` and reach.  Needs no library."""
    R = _branches(branches)
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    n = len(keys)
    G = _grouped(n, R)
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64).reshape(-1)
    if rho.shape != (n,):
        raise ValueError(f"rho must hold one value per frame ({n}), got {rho.size}")
    if np.size(scale) != G:
        raise ValueError(f"scale must hold one value per group ({G}), got {np.size(scale)}")
    gi, gq, x = _sent(cfg, keys[::R])                                             # one transmission per group: the leader's key
    c = p = reach = 0.0
    for r in range(R):                                                           # in increasing r, starting from 0
        c_r, p_r, reach_r = _branch(cfg, keys[r::R], H[r::R], E[r::R], sigma[r::R], x)
        w = rho[r::R, None, None]
        c, p, reach = c + w * c_r, p + w * p_r, reach + w * reach_r
    hard = _hard(cfg, gi, gq, c, p, reach, tau)
    soft = _soft(cfg, gi, gq, c, p, reach, scale, factors, e_lambda)
    return ((hard,) if tau is None else hard[:1]) + soft[:2] + (() if tau is None else hard[1:]) + soft[2:]


# ---- the decision-directed observation (module docstring, "the decision-directed observation"), mirrored by csrc/k_linkobserve.hip ----

OBSERVE_SOURCES = {"decided": _abi.AFT_LINK_OBSERVE_DECIDED, "sent": _abi.AFT_LINK_OBSERVE_SENT}
# What the decision map reads at a pilot position.  At 8 bits per symbol ki = kq = 15 is a legal decision with the same byte: the
# encoding is the interface's (ki | kq << 4, 255 at the pilots), so at m = 8 a reader tells the two apart by the pilot positions, as
# link_observe_host(decisions=) does with the data mask.
PILOT_DECISION = 255


def data_noise_scale(m: int) -> float:
    """The mean of ``1 / |a|^2`` over the unit-energy constellation of ``m`` bits per symbol: the factor by which dividing a received
    sample by its symbol raises the noise variance, on average.  1 for QPSK, 17/9 for 16-QAM."""
    return float(np.mean(1.0 / np.abs(constellation(m)) ** 2))


def _source(source) -> int:
    if not isinstance(source, str) or source not in OBSERVE_SOURCES:
        raise ValueError(f'source = {source!r}: "decided" (the receiver\'s own hard decisions) or "sent" (the sent symbols: the genie bound)')
    return OBSERVE_SOURCES[source]


def link_observe_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, pilots, branches: int = 1, source: str = "decided", decisions=None,
                      tau: Optional[float] = None):
    """The decision-directed observation (module docstring) in float64: ``keys`` / ``ideal`` / ``est`` / ``sigma`` / ``rho`` as
    ``link_mrc_host``'s for the ``n`` frames, ``pilots`` complex ``[n, Ps, Pt]`` the frames' noisy pilots -> ``(z complex128 [n, S, T],
    decisions uint8 [G, S, T], symbol_errors int64 [G])``, ``G = n / branches``.  The decision is the diversity link's own, on ``c = sum
    rho_r y_r conj(E_r)`` and ``p = sum rho_r |E_r|^2``; the map holds ``ki | kq << 4`` and 255 at the pilots (at ``m = 8`` the byte 255 is also the legal decision ``ki = kq = 15``: the pilot
    positions, not the byte, say which it is); ``symbol_errors`` counts the
    data elements whose level indices differ from the sent ones.  ``z_r = y_r conj(x^) / |x^|^2`` at a data element with ``x^`` the
    decided symbol -- the sent one with ``source="sent"`` (the map and the count stay the decided ones) -- and frame ``r``'s own pilot
    at a pilot position.  ``decisions=`` takes a given map in the map's own encoding instead of deciding (what a decoder that
    re-modulates would pass, and what a test passes to compare ``z`` on the device's own decisions); the map and the count returned
    are then the given one's.  With ``tau`` the flags ``[G, S, T, 2]`` of ``link_mrc_host`` on the same ``c``, ``p`` and reach follow.
    Needs no library."""
    R = _branches(branches)
    sent_source = _source(source) == OBSERVE_SOURCES["sent"]
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    n, (S, T), (Ps, Pt) = len(keys), cfg.sim.ofdm, cfg.sim.pilot
    G = _grouped(n, R)
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64).reshape(-1)
    if rho.shape != (n,):
        raise ValueError(f"rho must hold one value per frame ({n}), got {rho.size}")
    pilots = np.asarray(pilots).astype(np.complex128)
    if pilots.shape != (n, Ps, Pt):
        raise ValueError(f"Expected pilots of shape ({n}, {Ps}, {Pt}), got {pilots.shape}")
    L, d, mask = cfg.levels, cfg.d, cfg.data_mask
    gi, gq, x = _sent(cfg, keys[::R])                                             # one transmission per group: the leader's key
    y = np.empty((n, S, T), dtype=np.complex128)
    c = p = reach = 0.0
    for r in range(R):                                                           # in increasing r, starting from 0
        noise = _noise(cfg, keys[r::R], sigma[r::R])
        y[r::R] = H[r::R] * x + noise
        E_r, w = E[r::R], rho[r::R, None, None]
        c = c + w * (y[r::R] * E_r.conj())
        p = p + w * (E_r.real ** 2 + E_r.imag ** 2)
        reach = reach + w * ((np.abs(H[r::R]) * np.abs(x) + np.abs(noise)) * np.abs(E_r))
    if decisions is None:
        ki, kq = _levels(cfg, c.real, p), _levels(cfg, c.imag, p)
    else:
        given = np.asarray(decisions)
        if given.shape != (G, S, T) or given.dtype != np.uint8:
            raise ValueError(f"decisions must be uint8 [{G}, {S}, {T}] (ki | kq << 4, {PILOT_DECISION} at the pilots), got {given.dtype} "
                             f"{given.shape}")
        ki, kq = (given & 15).astype(np.int64), (given >> 4).astype(np.int64)
        if (np.maximum(ki, kq)[:, mask] >= L).any():
            raise ValueError(f"decisions holds a level index beyond the {L} levels of an axis at a data element")
    out = np.where(mask[None], ki | (kq << 4), PILOT_DECISION).astype(np.uint8)
    errors = (((ki != gray_level(gi)) | (kq != gray_level(gq))) & mask[None]).sum(axis=(1, 2)).astype(np.int64)
    xh = x if sent_source else d * ((2 * ki - (L - 1)) + 1j * (2 * kq - (L - 1)))
    xh = np.where(mask[None], xh, 1.0)                                            # a pilot position is not divided
    z = y * np.repeat((xh.conj() / np.abs(xh) ** 2), R, axis=0)
    sc, sym = np.asarray(cfg.sim.pilot_scs), np.asarray(cfg.sim.pilot_symbols)
    z[:, sc[:, None], sym[None, :]] = pilots
    if tau is None:
        return z, out, errors
    return z, out, errors, _hard(cfg, gi, gq, c, p, reach, tau)[2]


MAX_STREAMS = _abi.AFT_LINK_MAX_STREAMS
DETECTORS = ("zf", "mmse")


def _streams(streams) -> int:
    if isinstance(streams, bool) or not isinstance(streams, (int, np.integer)) or int(streams) != MAX_STREAMS:
        raise ValueError(f"streams = {streams!r}: the spatial-multiplexing link separates {MAX_STREAMS} streams")
    return int(streams)


def _sm_shape(n: int, branches, streams) -> Tuple[int, int, int]:
    """``(G, R, N)`` of a spatial-multiplexing batch of ``n`` frames, checked."""
    N, R = _streams(streams), _branches(branches)
    if R < 2:
        raise ValueError(f"branches = {R}: one antenna cannot separate {N} streams; an integer in 2 .. {MAX_BRANCHES}")
    return _grouped(n, R, N), R, N


def detector_reg(scale, detector: str) -> np.ndarray:
    """The regulariser float32 ``[G]`` of the leaders' float32 LLR scales: 0 for ``"zf"``, ``float32(1 / scale)`` (formed in double,
    rounded once) for ``"mmse"``."""
    if detector not in DETECTORS:
        raise ValueError(f"detector = {detector!r}: one of {DETECTORS}")
    scale = np.asarray(scale, dtype=np.float32).reshape(-1)
    if detector == "zf":
        return np.zeros_like(scale)
    return (1.0 / scale.astype(np.float64)).astype(np.float32)


def sm_weights(snr_db, err_var: float = 0.0, branches: int = 2, streams: int = 2, detector: str = "mmse"):
    """The detector's operands for frames at ``snr_db`` ``[n]`` in the spatial-multiplexing layout: ``(rho float32 [n], scale float32 [G],
    reg float32 [G])``: ``branch_weights`` over the ``branches * streams`` frames of a group (the entries of frames ``(r, 1)`` are not
    read) and ``detector_reg`` of the leaders' scale."""
    n = np.size(snr_db)
    _, R, N = _sm_shape(n, branches, streams)
    rho, scale = _weights(llr_scale(np.asarray(snr_db, dtype=np.float64).reshape(-1), err_var), R * N)
    return rho, scale, detector_reg(scale, detector)


def link_sm_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, scale, reg, branches, streams=2, factors=(1.0,),
                 tau: Optional[float] = None, e_lambda: Optional[float] = None):
    """The spatial-multiplexing link (module docstring) in float64: ``keys`` / ``ideal`` / ``est`` / ``sigma`` as ``link_errors_host``'s
    for the ``n`` frames in the layout ``g N R + r N + s``, ``rho`` ``[n]``, ``scale`` and ``reg`` ``[G]`` taken as the float32 numbers they
    are (``sm_weights``), ``G = n / (branches streams)`` -> ``(counts int64 [G, N, 2], loss float64 [G, N, K], llr float64
    [G, N, S, T, m])``.  With ``tau`` the wrong-bit map ``[G, N, S, T]`` and the flags ``[G, N, S, T, 2]`` follow, with ``e_lambda`` then
    ``loss_lo``, ``loss_hi`` and ``q``: the extras of ``link_mrc_host``, in its order, on the detector's ``c_s``, ``p_s``, reaches and
    ``eff_s``.  Needs no library."""
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    (G, R, N, S, T), sent, m, gss, rm, g01, G01, scale = _sm_sums(cfg, keys, H, E, sigma, rho, scale, branches, streams)
    if np.size(reg) != G:
        raise ValueError(f"reg must hold one value per group ({G}), got {np.size(reg)}")
    reg = np.asarray(reg, dtype=np.float32).astype(np.float64).reshape(G, 1, 1)
    a = [gss[0] + reg, gss[1] + reg]
    n01 = g01.real ** 2 + g01.imag ** 2
    c = np.stack([a[1] * m[0] - g01 * m[1], a[0] * m[1] - g01.conj() * m[0]], axis=1)              # [G, N, S, T]
    p = np.stack([gss[0] * a[1] - n01, gss[1] * a[0] - n01], axis=1)
    reach = np.stack([a[1] * rm[0] + G01 * rm[1], a[0] * rm[1] + G01 * rm[0]], axis=1)
    P = np.stack([gss[0] * a[1] + G01 ** 2, gss[1] * a[0] + G01 ** 2], axis=1)
    other = np.stack([a[1], a[0]], axis=1)
    eff = np.divide(np.broadcast_to(scale[:, None], other.shape), other, out=np.zeros_like(other), where=other > 0)
    flat = lambda v: v.reshape(G * N, S, T)  # noqa: E731
    gi, gq = (flat(np.stack([sent[0][i], sent[1][i]], axis=1)) for i in (0, 1))
    hard = _hard(cfg, gi, gq, flat(c), flat(p), flat(reach), tau, flat(P))
    soft = _soft(cfg, gi, gq, flat(c), flat(p), flat(reach), flat(eff), factors, e_lambda, flat(P))
    out = ((hard,) if tau is None else hard[:1]) + soft[:2] + (() if tau is None else hard[1:]) + soft[2:]
    return tuple(v.reshape(G, N, *v.shape[1:]) for v in out)


def _sm_sums(cfg: LinkConfig, keys, H, E, sigma, rho, scale, branches, streams):
    """What the two-stream definitions share, on checked operands: ``((G, R, N, S, T), sent, m, gss, rm, g01, G01, scale)`` -- the sent
    words ``(gi, gq, x)`` per stream, the matched sums ``m_s``, the Gram sums ``g_ss`` and ``g01``, the reaches ``reach(m_s)`` and ``G01``,
    each ``[G, S, T]``, and the leaders' scale as float64 ``[G, 1, 1]``."""
    n, (S, T) = len(keys), cfg.sim.ofdm
    G, R, N = _sm_shape(n, branches, streams)
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64).reshape(-1)
    if rho.shape != (n,):
        raise ValueError(f"rho must hold one value per frame ({n}), got {rho.size}")
    if np.size(scale) != G:
        raise ValueError(f"scale must hold one value per group ({G}), got {np.size(scale)}")
    scale = np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(G, 1, 1)
    keys, sigma, rho = keys.reshape(G, R, N), sigma.reshape(G, R, N), rho.reshape(G, R, N)
    H, E = H.reshape(G, R, N, S, T), E.reshape(G, R, N, S, T)
    sent = [_sent(cfg, np.ascontiguousarray(keys[:, 0, s])) for s in range(N)]   # one transmission per stream: the keys of frames (0, s)
    x0, x1 = sent[0][2], sent[1][2]
    m, gss, rm = [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]
    g01 = G01 = 0.0
    for r in range(R):                                                           # in increasing r, starting from 0
        noise = _noise(cfg, np.ascontiguousarray(keys[:, r, 0]), sigma[:, r, 0])
        y = H[:, r, 0] * x0 + H[:, r, 1] * x1 + noise
        ry = np.abs(H[:, r, 0]) * np.abs(x0) + np.abs(H[:, r, 1]) * np.abs(x1) + np.abs(noise)
        w = rho[:, r, 0, None, None]
        for s in range(N):
            e = E[:, r, s]
            m[s] = m[s] + w * (y * e.conj())
            gss[s] = gss[s] + w * (e.real ** 2 + e.imag ** 2)
            rm[s] = rm[s] + w * (ry * np.abs(e))
        g01 = g01 + w * (E[:, r, 0].conj() * E[:, r, 1])
        G01 = G01 + w * (np.abs(E[:, r, 0]) * np.abs(E[:, r, 1]))
    return (G, R, N, S, T), sent, m, gss, rm, g01, G01, scale


JOINT_DETECTOR = "joint"
ALL_DETECTORS = DETECTORS + (JOINT_DETECTOR,)


def _detector(detector) -> str:
    """A detector's name, checked: the linear ones by ``detector_reg`` (which keeps refusing everything else), ``"joint"`` or
    ``"sic"``."""
    if not (isinstance(detector, str) and detector in (JOINT_DETECTOR, "sic")):
        detector_reg(np.ones(1, np.float32), detector)
    return detector


def link_joint_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, scale, branches, streams=2, factors=(1.0,),
                    tau: Optional[float] = None, e_lambda: Optional[float] = None):
    """The joint link (module docstring) in float64: the operands of ``link_sm_host`` without ``reg`` -> ``link_sm_host``'s tuple, in its
    order: ``(counts int64 [G, N, 2], loss float64 [G, N, K], llr float64 [G, N, S, T, m])``; with ``tau`` the wrong-bit map
    ``[G, N, S, T]`` and the flags ``[G, N, S, T, m]`` (a data (element, stream, bit) with ``|Delta_j| <= tau Q``) follow, with ``e_lambda``
    then ``loss_lo``, ``loss_hi`` (the losses at ``Lambda -+ e_lambda q``) and ``q = scale Q`` ``[G, N, S, T, m]``, 0 at the pilots.  Needs
    no library."""
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    (G, R, N, S, T), sent, ms, gss, rm, g01, G01, scale = _sm_sums(cfg, keys, H, E, sigma, rho, scale, branches, streams)
    m, L, d = cfg.bits_per_symbol, cfg.levels, cfg.d
    half = m // 2
    factors = _factors(factors).astype(np.float64)
    a = d * (2 * np.arange(L) - (L - 1))
    A = (L - 1) * d
    zero = np.zeros((G, S, T))                                                   # a batch of all-pilot grids keeps its shapes
    mu = lambda comp, p: a * (a * p[..., None] - 2.0 * comp[..., None])  # noqa: E731     [..., L]: the soft link's metric
    delta = np.empty((G, N, S, T, m))
    for e in range(N):
        o = 1 - e
        g_oe = (g01 if e == 1 else np.conj(g01)) + zero
        m_e, m_o, g_ee, g_oo = ms[e] + zero, ms[o] + zero, gss[e] + zero, gss[o] + zero
        t_i, t_q = mu(m_e.real, g_ee), mu(m_e.imag, g_ee)                          # g_ee a^2 - 2 a comp, per axis
        f = np.empty((G, S, T, L, L))                                             # [.., ki, kq]
        for ki in range(L):
            z = m_o[..., None] - g_oe[..., None] * (a[ki] + 1j * a)               # [G, S, T, kq]
            r = mu(z.real, g_oo[..., None]).min(axis=-1) + mu(z.imag, g_oo[..., None]).min(axis=-1)
            f[..., ki, :] = (t_i[..., ki, None] + t_q) + r
        rows, cols = f.min(axis=-1), f.min(axis=-2)                               # over kq: the I axis's; over ki: the Q axis's
        for axis, best in enumerate((rows, cols)):
            for j, split in enumerate(_gray_split(best, half)):
                delta[:, e, ..., axis * half + j] = split
    mask = cfg.data_mask[None, None, :, :, None]
    delta *= mask
    llr = delta * scale[:, None, :, :, None]
    gi, gq = (np.stack([sent[0][i], sent[1][i]], axis=1) for i in (0, 1))         # [G, N, S, T]
    sign = _sent_signs(gi, gq, half)                                              # 1 - 2 b_j
    wrong = (((llr < 0) != (sign < 0)) & (mask != 0)).sum(axis=-1)                # the sign rule against the sent bits
    counts = np.stack([wrong.sum(axis=(2, 3)), (wrong > 0).sum(axis=(2, 3))], axis=-1).astype(np.int64)

    losses = _losses_at(sign, mask, factors)
    out = (counts, losses(llr), llr)
    if tau is None and e_lambda is None:
        return out
    Q = (2.0 * A * A * (gss[0] + gss[1] + 2.0 * G01) + 2.0 * np.sqrt(2.0) * A * (rm[0] + rm[1])) + zero
    Q = np.broadcast_to(Q[:, None, :, :, None], delta.shape) * mask
    if tau is not None:
        out += (wrong, (np.abs(delta) <= tau * Q) & (mask != 0))
    if e_lambda is not None:
        q = scale[:, None, :, :, None] * Q
        out += (losses(llr + sign * (e_lambda * q)), losses(llr - sign * (e_lambda * q)), q)
    return out


# ---- the successive-cancellation link (module docstring, "The successive-cancellation link"): float64 NumPy, mirrored by csrc/k_linksm.hip ----

SIC_DETECTOR = "sic"
LINK2_DETECTORS = ALL_DETECTORS + (SIC_DETECTOR,)           # every detector of the two-stream link; ALL_DETECTORS stays the first three
SIC_STATS = 3                                               # swapped order, first-decision symbol errors, of those the propagated ones


def _levels(cfg: LinkConfig, comp: np.ndarray, p: np.ndarray) -> np.ndarray:
    """The decided level index of an axis: ``#{b in 1 .. L-1 : comp >= beta_b p}``."""
    L, d = cfg.levels, cfg.d
    level = np.zeros(comp.shape, dtype=np.int64)
    for b in range(1, L):
        level += comp >= (2.0 * d * (b - L / 2)) * p
    return level


def link_sic_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, scale, reg, branches, streams=2, factors=(1.0,),
                  tau: Optional[float] = None, e_lambda: Optional[float] = None, genie: bool = False):
    """The successive-cancellation link (module docstring) in float64: the operands of ``link_sm_host``, ``reg`` any float32 ``>= 0`` per
    group -> ``(counts int64 [G, N, 2], loss float64 [G, N, K], llr float64 [G, N, S, T, m], stats int64 [G, 3])``, the first three
    indexed by stream.  With ``tau`` the wrong-bit map ``[G, N, S, T]``, the flags ``[G, N, S, T, 2]`` (the first-detected stream's by the
    spatial-multiplexing link's margin, the other stream's by the diversity link's on ``(c_o, p_o)``) and the dependent map uint8
    ``[G, S, T]`` follow: 0, 1 at a dependent element (there the SECOND stream's outputs may differ freely) and 2 at an order-flagged
    one (there both streams' may).  With ``e_lambda`` then ``loss_lo``, ``loss_hi`` and ``q [G, N, S, T, m]``: at a dependent (element,
    stream) ``q`` is ``q_dep`` (at an order-flagged element the larger of ``q_dep`` and the linear detector's ``q``), the LLR is only
    known to lie within ``2 q (1 + e_lambda)`` of 0, and the loss interval takes those two ends.  ``genie=True`` cancels the SENT symbol
    of the first stream instead of the decided one: the propagation-free bound.  Needs no library."""
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    (G, R, N, S, T), sent, ms, gss, rm, g01, G01, scale = _sm_sums(cfg, keys, H, E, sigma, rho, scale, branches, streams)
    if np.size(reg) != G:
        raise ValueError(f"reg must hold one value per group ({G}), got {np.size(reg)}")
    reg = np.asarray(reg, dtype=np.float32).astype(np.float64).reshape(G, 1, 1)
    m, L, d = cfg.bits_per_symbol, cfg.levels, cfg.d
    half, A = m // 2, (L - 1) * d
    zero = np.zeros((G, S, T))                                                   # a batch of all-pilot grids keeps its shapes
    ms, gss, rm = [v + zero for v in ms], [v + zero for v in gss], [v + zero for v in rm]
    g01, G01, scale = g01 + zero, G01 + zero, scale + zero
    # the linear detector of both streams, as link_sm_host forms it
    a = [gss[0] + reg, gss[1] + reg]
    n01 = g01.real ** 2 + g01.imag ** 2
    c_lin = [a[1] * ms[0] - g01 * ms[1], a[0] * ms[1] - g01.conj() * ms[0]]
    p_lin = [gss[0] * a[1] - n01, gss[1] * a[0] - n01]
    reach_lin = [a[1] * rm[0] + G01 * rm[1], a[0] * rm[1] + G01 * rm[0]]
    P_lin = [gss[0] * a[1] + G01 ** 2, gss[1] * a[0] + G01 ** 2]
    eff = [np.divide(scale, a[1 - s], out=np.zeros_like(zero), where=a[1 - s] > 0) for s in range(N)]
    with np.errstate(invalid="ignore"):
        f = gss[1] > gss[0]                                                      # stream 1 first; a tie and NaN give stream 0
    pick = lambda v: np.where(f, v[1], v[0])  # noqa: E731                        the first-detected stream's
    other = lambda v: np.where(f, v[0], v[1])  # noqa: E731                       the second's
    c_f, p_f = pick(c_lin), pick(p_lin)
    if genie:
        xhat = pick([sent[0][2], sent[1][2]])
    else:
        xhat = d * ((2 * _levels(cfg, c_f.real, p_f) - (L - 1)) + 1j * (2 * _levels(cfg, c_f.imag, p_f) - (L - 1)))
    gx = np.where(f, g01, g01.conj())                                            # g01 when the other stream is 0
    c_o, p_o, reach_o = other(ms) - gx * xhat, other(gss), other(rm) + G01 * np.abs(xhat)
    first = np.stack([~f, f], axis=1)                                            # [G, N, S, T]: stream s is the first-detected one
    by_stream = lambda lin, sec: np.where(first, np.stack(lin, axis=1), sec[:, None])  # noqa: E731
    c, p, reach = by_stream(c_lin, c_o), by_stream(p_lin, p_o), by_stream(reach_lin, reach_o)
    p_reach, sc = by_stream(P_lin, p_o), by_stream(eff, scale)
    flat = lambda v: v.reshape(G * N, S, T)  # noqa: E731
    gi, gq = (np.stack([sent[0][i], sent[1][i]], axis=1) for i in (0, 1))         # [G, N, S, T]
    counts, wrong, flags = _hard(cfg, flat(gi), flat(gq), flat(c), flat(p), flat(reach), -1.0 if tau is None else tau, flat(p_reach))
    loss, llr = _soft(cfg, flat(gi), flat(gq), flat(c), flat(p), flat(reach), flat(sc), factors, None, flat(p_reach))
    counts, wrong, flags, loss, llr = (v.reshape(G, N, *v.shape[1:]) for v in (counts, wrong, flags, loss, llr))
    mask = cfg.data_mask[None]
    wrong_f, wrong_o = np.where(f, wrong[:, 1], wrong[:, 0]), np.where(f, wrong[:, 0], wrong[:, 1])
    stats = np.stack([(f & mask).sum(axis=(1, 2)), (wrong_f > 0).sum(axis=(1, 2)), ((wrong_f > 0) & (wrong_o > 0)).sum(axis=(1, 2))],
                     axis=1).astype(np.int64)
    out = (counts, loss, llr, stats)
    if tau is None and e_lambda is None:
        return out
    t = 0.0 if tau is None else tau
    order = (np.abs(gss[0] - gss[1]) <= t * (gss[0] + gss[1])) & mask            # the order itself may differ
    dependent = order | (np.where(first, flags.any(axis=-1), False).any(axis=1) & mask)
    if tau is not None:
        out += (wrong, flags, dependent.astype(np.uint8) + order)
    if e_lambda is not None:
        q_own = sc * A * (A * p_reach + 2.0 * reach)
        q_lin = np.stack(eff, axis=1) * A * (A * np.stack(P_lin, axis=1) + 2.0 * np.stack(reach_lin, axis=1))
        q_dep = scale[:, None] * A * (A * np.stack(gss, axis=1) + 2.0 * (np.stack(rm, axis=1) + np.sqrt(2.0) * A * G01[:, None]))
        free = (dependent[:, None] & ~first) | order[:, None]                    # [G, N, S, T]: this stream's outputs may differ freely
        q = np.where(free, np.where(order[:, None], np.maximum(q_lin, q_dep), q_dep), q_own) * mask[:, None]
        q = np.broadcast_to(q[..., None], llr.shape).copy()
        sign = _sent_signs(gi, gq, half)
        losses = _losses_at(sign, cfg.data_mask[None, None, :, :, None], _factors(factors).astype(np.float64))
        end = 2.0 * q * (1.0 + e_lambda)
        toward = np.where(free[..., None], sign * end, llr + sign * (e_lambda * q))
        away = np.where(free[..., None], -sign * end, llr - sign * (e_lambda * q))
        out += (losses(toward), losses(away), q)
    return out


# ---- the codeword-cancellation link (module docstring, "The codeword-cancellation link"): float64 / integer NumPy, mirrored by
# ---- csrc/k_linksm.hip (the cancel detector) and csrc/k_linkldpc.hip (the masked decoder) ----

CWSIC_DETECTOR = "cwsic"
#: every name ``detector=`` takes somewhere; ``"cwsic"`` only on ``LdpcBlockErrorAccumulator`` and ``evaluation.get_link_bler``
CODED_DETECTORS = LINK2_DETECTORS + (CWSIC_DETECTOR,)
_CWSIC_ONLY = ('detector="cwsic" decodes between its two detections: it runs on LdpcBlockErrorAccumulator(code, device, branches=R, '
               'streams=2, detector="cwsic") and evaluation.get_link_bler(..., detector="cwsic") with an LdpcConfig only')


def _refuse_cwsic(detector, what: str, instead: str) -> None:
    if isinstance(detector, str) and detector == CWSIC_DETECTOR:
        raise ValueError(f'{what} has no detector="cwsic": {_CWSIC_ONLY}; {instead}')


def cwsic_redetect(failed) -> np.ndarray:
    """Step 2 of the codeword-cancellation link: ``failed`` ``[..., 2]`` (anything non-zero counts as failed: block-error counts do) ->
    bool ``[..., 2]``, ``redo[..., s] = failed[..., s] and not failed[..., 1 - s]``.  At most one stream of a group is set."""
    failed = np.asarray(failed) != 0
    if failed.ndim < 1 or failed.shape[-1] != MAX_STREAMS:
        raise ValueError(f"failed must hold {MAX_STREAMS} streams on its last axis, got shape {failed.shape}")
    return failed & ~failed[..., ::-1]


def link_cancel_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, scale, branches, redo, streams=2, factors=(1.0,),
                     tau: Optional[float] = None, e_lambda: Optional[float] = None):
    """Step 3 of the codeword-cancellation link (module docstring) in float64: the operands of ``link_sm_host`` without ``reg``, and
    ``redo`` bool ``[G, N]`` (``cwsic_redetect``; at most one stream per group) -> ``(counts int64 [G, N, 2], loss float64 [G, N, K], llr
    float64 [G, N, S, T, m])``, all zeros for a stream without ``redo``.  With ``tau`` the wrong-bit map ``[G, N, S, T]`` and the flags
    ``[G, N, S, T, 2]`` follow, with ``e_lambda`` then ``loss_lo``, ``loss_hi`` and ``q``: what ``link_sic_host`` returns for its second
    stream, on ``reach = reach(m_s) + G01 |x_o|`` and ``p_reach = g_ss``; zeros (False) without ``redo``.  Needs no library."""
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    (G, R, N, S, T), sent, ms, gss, rm, g01, G01, scale = _sm_sums(cfg, keys, H, E, sigma, rho, scale, branches, streams)
    redo = np.asarray(redo)
    if redo.shape != (G, N) or redo.dtype != np.bool_:
        raise ValueError(f"redo must be bool of shape ({G}, {N}), got {redo.dtype} {redo.shape}")
    if (redo.sum(axis=1) > 1).any():
        raise ValueError("redo: at most one stream of a group is detected again (cwsic_redetect)")
    zero = np.zeros((G, S, T))                                                   # a batch of all-pilot grids keeps its shapes
    c = np.stack([(ms[0] + zero) - g01 * sent[1][2], (ms[1] + zero) - np.conj(g01) * sent[0][2]], axis=1)    # m_s - g_so x_o
    p = np.stack([gss[0] + zero, gss[1] + zero], axis=1)
    reach = np.stack([(rm[0] + zero) + G01 * np.abs(sent[1][2]), (rm[1] + zero) + G01 * np.abs(sent[0][2])], axis=1)
    sc = np.broadcast_to((scale + zero)[:, None], c.shape)
    flat = lambda v: np.ascontiguousarray(v).reshape(G * N, S, T)  # noqa: E731
    gi, gq = (flat(np.stack([sent[0][i], sent[1][i]], axis=1)) for i in (0, 1))
    hard = _hard(cfg, gi, gq, flat(c), flat(p), flat(reach), tau)
    soft = _soft(cfg, gi, gq, flat(c), flat(p), flat(reach), flat(sc), factors, e_lambda)
    out = ((hard,) if tau is None else hard[:1]) + soft[:2] + (() if tau is None else hard[1:]) + soft[2:]
    out = tuple(v.reshape(G, N, *v.shape[1:]) for v in out)
    keep = lambda v: np.where(redo.reshape(G, N, *(1,) * (v.ndim - 2)), v, np.zeros((), v.dtype))  # noqa: E731   without redo: zeros
    return tuple(keep(v) for v in out)


def link_cwsic_host(code: "LdpcConfig", keys, ideal, est, sigma, rho, scale, reg, branches):
    """The codeword-cancellation link (module docstring) on its host twins: the operands of ``link_sm_host`` for the two streams, ``reg``
    the first pass's (``detector_reg(scale, "mmse")`` by the definition) -> ``(first int64 [G, 2, 3], redo bool [G, 2], second int64
    [G, 2, 3], final int64 [G, 2, 3])``: the decoder's counts (information-bit errors, block errors, iterations) of the first pass,
    the flags, the second pass's counts (zeros without ``redo``) and the final ones -- the second pass's bit and block errors where
    ``redo``, the first pass's elsewhere, the iterations of both passes summed.  Needs no library."""
    if not isinstance(code, LdpcConfig):
        raise ValueError(f"link_cwsic_host needs an LdpcConfig (got {type(code).__name__})")
    cfg = code.link
    llr = link_sm_host(cfg, keys, ideal, est, sigma, rho, scale, reg, branches)[2]
    G, N = llr.shape[:2]
    sent_keys = np.ascontiguousarray(_keys64(keys).reshape(G, -1, N)[:, 0, :]).reshape(-1)       # the keys of frames (0, s)
    first = link_ldpc_host(code, sent_keys, llr.reshape(G * N, *llr.shape[2:]))[0].reshape(G, N, 3)
    redo = cwsic_redetect(first[..., 1])
    second = np.zeros_like(first)
    if redo.any():                                                               # decode the streams detected again, and only them
        again = link_cancel_host(cfg, keys, ideal, est, sigma, rho, scale, branches, redo)[2]
        pick = redo.reshape(-1)
        second.reshape(G * N, 3)[pick] = link_ldpc_host(code, sent_keys[pick], again.reshape(G * N, *again.shape[2:])[pick])[0]
    return first, redo, second, cwsic_final(first, redo, second)


def cwsic_final(first, redo, second) -> np.ndarray:
    """Step 4: the second pass's bit and block errors where ``redo``, the first pass's elsewhere; the iterations of both passes."""
    first, second = np.asarray(first), np.asarray(second)
    final = np.where(np.asarray(redo, dtype=bool)[..., None], second, first)
    final[..., 2] = first[..., 2] + second[..., 2]
    return final


# ---- the transmit-diversity link (module docstring, "The transmit-diversity link"): float64 NumPy, mirrored by csrc/k_linkalamouti.hip ----

PAIRINGS = ("time", "frequency")


def _pairing(pairing) -> int:
    """The library's constant of a pairing's name, checked."""
    if not isinstance(pairing, str) or pairing not in PAIRINGS:
        raise ValueError(f"pairing = {pairing!r}: one of {PAIRINGS}")
    return (_abi.AFT_LINK_PAIR_TIME, _abi.AFT_LINK_PAIR_FREQUENCY)[PAIRINGS.index(pairing)]


def _tx_grouped(n: int, branches: int) -> int:
    if n % (branches * 2):
        raise ValueError(f"a batch of {n} frames is not a multiple of branches * 2 = {branches} * 2")
    return n // (branches * 2)


def alamouti_pairs(cfg: LinkConfig, pairing: str = "time") -> Tuple[np.ndarray, np.ndarray]:
    """The Alamouti pairs of a grid: ``(role int8 [S, T], partner int64 [S, T])``.  ``role`` is -1 at a pilot, 0 at the first element
    of a pair, 1 at its second and 2 at a lone element; ``partner`` is the flat index ``s T + t`` of the other element of the pair, and
    a pilot's or a lone element's own.  A line is a subcarrier for ``"time"`` and a symbol for ``"frequency"``; its data elements in
    increasing order pair up two by two, whether or not pilots lie between them."""
    _pairing(pairing)
    S, T = cfg.sim.ofdm
    mask = cfg.data_mask
    flat = np.arange(S * T, dtype=np.int64).reshape(S, T)
    role, partner = np.full((S, T), -1, dtype=np.int8), flat.copy()
    if pairing == "frequency":                                                   # the lines are the columns: work on the transposed views
        mask, flat, role_v, partner_v = mask.T, flat.T, role.T, partner.T
    else:
        role_v, partner_v = role, partner
    for line in range(mask.shape[0]):
        data = np.flatnonzero(mask[line])
        pairs = len(data) // 2
        a, b = data[0:2 * pairs:2], data[1:2 * pairs:2]
        role_v[line, a], role_v[line, b] = 0, 1
        partner_v[line, a], partner_v[line, b] = flat[line, b], flat[line, a]
        if len(data) % 2:
            role_v[line, data[-1]] = 2
    return role, partner


def alamouti_weights(snr_db, err_var: float = 0.0, branches: int = 1) -> Tuple[np.ndarray, np.ndarray]:
    """The combiner's operands for frames at ``snr_db`` ``[n]`` in the transmit-diversity layout: ``(rho float32 [n], scale float32
    [G])``, ``branch_weights`` over the ``2 * branches`` frames of a group (the entries of frames ``(r, 1)`` are not read)."""
    R = _branches(branches)
    snr = np.asarray(snr_db, dtype=np.float64).reshape(-1)
    _tx_grouped(snr.size, R)
    return _weights(llr_scale(snr, err_var), 2 * R)


def link_alamouti_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, scale, branches, pairing: str = "time", factors=(1.0,),
                       tau: Optional[float] = None, e_lambda: Optional[float] = None):
    """The transmit-diversity link (module docstring) in float64: ``keys`` / ``ideal`` / ``est`` / ``sigma`` as ``link_errors_host``'s
    for the ``n`` frames in the layout ``g 2R + r 2 + s``, ``rho`` ``[n]`` and ``scale`` ``[G]`` taken as the float32 numbers they are
    (``alamouti_weights``), ``G = n / (2 branches)`` -> ``link_mrc_host``'s tuple, in its order: ``(counts int64 [G, 2], loss float64
    [G, K], llr float64 [G, S, T, m])``; with ``tau`` the wrong-bit map ``[G, S, T]`` and the flags ``[G, S, T, 2]`` follow, with
    ``e_lambda`` then ``loss_lo``, ``loss_hi`` and ``q``, on the combiner's ``c``, ``p`` and reach.  Needs no library."""
    R = _branches(branches)
    role, partner = alamouti_pairs(cfg, pairing)
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    n, (S, T) = len(keys), cfg.sim.ofdm
    G = _tx_grouped(n, R)
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64).reshape(-1)
    if rho.shape != (n,):
        raise ValueError(f"rho must hold one value per frame ({n}), got {rho.size}")
    if np.size(scale) != G:
        raise ValueError(f"scale must hold one value per group ({G}), got {np.size(scale)}")
    W = 2 * R
    gi, gq, x = _sent(cfg, keys[::W])                                             # one transmission per group: the leader's key
    at = partner.reshape(-1)
    other = lambda v: v.reshape(G, S * T)[:, at].reshape(G, S, T)  # noqa: E731     a [G, S, T] array at every element's partner
    first, second = role == 0, role == 1                                          # pilots and lone elements: neither
    xo = other(x)
    # what the two antennas send at every element: (x_a, x_b) at a, (-conj(x_b), conj(x_a)) at b, (x, 0) at a lone element
    t0 = np.where(second, -np.conj(x), x)
    t1 = np.where(first, xo, np.where(second, np.conj(xo), 0.0))
    c = p = reach = 0.0
    for r in range(R):                                                           # in increasing r, starting from 0
        sl = slice(2 * r, None, W)                                               # the frames (r, 0); (r, 1) follow them
        H0, H1, E0, E1 = H[sl], H[2 * r + 1::W], E[sl], E[2 * r + 1::W]
        noise = _noise(cfg, keys[sl], sigma[sl])
        y = H0 * t0 + H1 * t1 + noise
        ry = np.abs(H0) * np.abs(t0) + np.abs(H1) * np.abs(t1) + np.abs(noise)
        yo, ryo, E0o, E1o = other(y), other(ry), other(E0), other(E1)
        n0, n1 = E0.real ** 2 + E0.imag ** 2, E1.real ** 2 + E1.imag ** 2
        # (the term at a, the term at b) of c, of p and of the reach, per role of the element
        # (y conj(E) in _branch's operand order: with H_r1 = E_r1 = 0 the first and lone elements are link_mrc_host's bit for bit)
        ca = np.where(second, yo * E1o.conj(), y * E0.conj())
        cb = np.where(first, yo.conj() * E1o, np.where(second, -(y.conj() * E0), 0.0))
        pa = np.where(second, other(n1), n0)
        pb = np.where(first, other(n1), np.where(second, n0, 0.0))
        ra = np.where(second, np.abs(E1o) * ryo, np.abs(E0) * ry)
        rb = np.where(first, np.abs(E1o) * ryo, np.where(second, np.abs(E0) * ry, 0.0))
        w = rho[sl, None, None]
        c, p, reach = (c + w * ca) + w * cb, (p + w * pa) + w * pb, (reach + w * ra) + w * rb
    hard = _hard(cfg, gi, gq, c, p, reach, tau)
    soft = _soft(cfg, gi, gq, c, p, reach, scale, factors, e_lambda)
    return ((hard,) if tau is None else hard[:1]) + soft[:2] + (() if tau is None else hard[1:]) + soft[2:]


# ---- the closed-loop link (module docstring, "The closed-loop link"): float64 NumPy, mirrored by csrc/k_linkprecode.hip ----

CODEBOOK = (1.0 + 0.0j, -1.0 + 0.0j, 1.0j, -1.0j)           # q_0 .. q_3; the precoder of index i is (1, q_i)
MAX_SUBBANDS = _abi.AFT_LINK_MAX_SUBBANDS

#: the weights of the closed-loop link: the same frames (r, 0) of the same groups of 2 R frames
precoding_weights = alamouti_weights


def _subband(cfg: LinkConfig, subband) -> int:
    """The subband width in subcarriers, checked against the grid."""
    S = cfg.sim.ofdm[0]
    if isinstance(subband, bool) or not isinstance(subband, (int, np.integer)) or not 1 <= int(subband) <= S:
        raise ValueError(f"precoding_subband = {subband!r}: an integer in 1 .. {S} subcarriers")
    if -(-S // int(subband)) > MAX_SUBBANDS:
        raise ValueError(f"precoding_subband = {subband} makes {-(-S // int(subband))} subbands of the {S} subcarriers, more than {MAX_SUBBANDS}")
    return int(subband)


def precoding_subbands(cfg: LinkConfig, subband: int) -> Tuple[np.ndarray, int]:
    """The subbands of a grid: ``(index int64 [S], n_sub)``, ``index[s] = s // subband`` the subband of subcarrier ``s`` and
    ``n_sub = ceil(S / subband)``; the last subband is short where ``subband`` does not divide ``S``."""
    B, S = _subband(cfg, subband), cfg.sim.ofdm[0]
    return np.arange(S, dtype=np.int64) // B, -(-S // B)


def _mul_q(i, z: np.ndarray) -> np.ndarray:
    """``q_i z`` for the codebook indices ``i`` (broadcast against ``z``): a swap and negations, exact."""
    i = np.broadcast_to(np.asarray(i, dtype=np.int64), z.shape)
    turn, neg = (i & 2) != 0, (i & 1) != 0
    re, im = np.where(turn, -z.imag, z.real), np.where(turn, z.real, z.imag)
    out = np.empty(z.shape, dtype=np.complex128)
    out.real, out.imag = np.where(neg, -re, re), np.where(neg, -im, im)
    return out


def _rho_of(rho, n: int) -> np.ndarray:
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64).reshape(-1)
    if rho.shape != (n,):
        raise ValueError(f"rho must hold one value per frame ({n}), got {rho.size}")
    return rho


def delayed_groups(groups: int, slots, delay) -> Tuple[np.ndarray, np.ndarray]:
    """Delayed feedback (module docstring) on ``groups`` input groups in sequences of ``slots``: ``(transmit, feedback)``, int64
    ``[groups / slots * (slots - delay)]`` each -- output group ``o = seq (K - d) + (k - d)`` sends input group ``seq K + k`` with the
    PMIs selected from input group ``seq K + k - d``."""
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (slots, delay)) or slots < 1 or not 0 <= delay < slots:
        raise ValueError(f"slots = {slots!r}, delay = {delay!r}: integers with slots >= 1 and 0 <= delay < slots")
    K, d = int(slots), int(delay)
    if groups % K:
        raise ValueError(f"{groups} groups are not whole sequences of slots = {K}")
    sent = (np.arange(groups // K, dtype=np.int64)[:, None] * K + np.arange(d, K, dtype=np.int64)[None, :]).reshape(-1)
    return sent, sent - d


def _group_frames(groups: np.ndarray, width: int) -> np.ndarray:
    """The frames of the given groups of ``width`` frames, in order."""
    return (groups[:, None] * width + np.arange(width, dtype=np.int64)[None, :]).reshape(-1)


def precoding_pmi_host(cfg: LinkConfig, est, rho, branches, subband, tau_pmi: Optional[float] = None, slots: int = 1, delay: int = 0):
    """The selection of the closed-loop link (module docstring) in float64: ``est`` complex ``[n, S, T]`` and ``rho`` ``[n]`` in the
    layout ``g 2R + r 2 + s`` -> ``pmi int32 [G, n_sub]``, per subband the lowest index that attains the maximum of ``Re(q_i g_b)``.
    With ``tau_pmi``: ``(pmi, flags bool [G, n_sub])``, the PMI-flagged subbands.  With ``slots`` / ``delay`` ("delayed feedback") the
    rows are the compact output groups': the selection on each transmitted slot's FEEDBACK group."""
    R = _branches(branches)
    if slots != 1 or delay != 0:
        E, rho = np.asarray(est), np.asarray(rho).reshape(-1)
        _, feedback = delayed_groups(_tx_grouped(E.shape[0], R), slots, delay)
        at = _group_frames(feedback, 2 * R)
        return precoding_pmi_host(cfg, E[at], rho[at], R, subband, tau_pmi)
    index, n_sub = precoding_subbands(cfg, subband)
    S, T = cfg.sim.ofdm
    E = np.asarray(est).astype(np.complex128)
    if E.ndim != 3 or E.shape[1:] != (S, T):
        raise ValueError(f"Expected est of shape (n, {S}, {T}), got {E.shape}")
    n = E.shape[0]
    G, W = _tx_grouped(n, R), 2 * R
    rho = _rho_of(rho, n)
    gr, gi, gross = np.zeros((G, S)), np.zeros((G, S)), np.zeros((G, S))        # per subcarrier: the sums over t and r
    for r in range(R):
        E0, E1, w = E[2 * r::W], E[2 * r + 1::W], rho[2 * r::W, None]
        gr += w * (E0.real * E1.real + E0.imag * E1.imag).sum(axis=2)             # conj(E_r0) E_r1
        gi += w * (E0.real * E1.imag - E0.imag * E1.real).sum(axis=2)
        gross += w * (np.abs(E0) * np.abs(E1)).sum(axis=2)
    starts = np.flatnonzero(np.diff(index, prepend=-1))
    gr, gi, gross = (np.add.reduceat(v, starts, axis=1) for v in (gr, gi, gross))
    v = np.stack([gr, -gr, -gi, gi], axis=-1)                                     # Re(q_i g_b)
    pmi = v.argmax(axis=-1).astype(np.int32)                                      # the first index that attains the maximum
    if tau_pmi is None:
        return pmi
    top = np.sort(v, axis=-1)
    return pmi, (top[..., 3] - top[..., 2]) <= tau_pmi * gross


def link_precoded_host(cfg: LinkConfig, keys, ideal, est, sigma, rho, scale, branches, subband, factors=(1.0,),
                       tau: Optional[float] = None, e_lambda: Optional[float] = None, pmi=None, slots: int = 1, delay: int = 0):
    """The closed-loop link (module docstring) in float64: ``keys`` / ``ideal`` / ``est`` / ``sigma`` as ``link_errors_host``'s for the
    ``n`` frames in the layout ``g 2R + r 2 + s``, ``rho`` ``[n]`` and ``scale`` ``[G]`` taken as the float32 numbers they are
    (``precoding_weights``), ``G = n / (2 branches)`` -> ``link_alamouti_host``'s tuple with ``pmi`` appended: ``(counts int64 [G, 2],
    loss float64 [G, K], llr float64 [G, S, T, m], pmi int32 [G, n_sub])``; with ``tau`` the wrong-bit map ``[G, S, T]`` and the flags
    ``[G, S, T, 2]`` follow the LLRs, with ``e_lambda`` then ``loss_lo``, ``loss_hi`` and ``q``, on the combiner's ``c``, ``p`` and
    reaches; ``pmi`` stays last.  A given ``pmi`` ``[G, n_sub]`` (values 0 .. 3) replaces the selection.  Needs no library.
    ``slots=K, delay=d`` is "delayed feedback" (module docstring): the ``G = Q K`` groups are Q sequences of K slots, slot ``k >= d`` is
    sent with the PMIs selected from ``est`` and ``rho`` of slot ``k - d``, and every output has the ``Q (K - d)`` compact rows; the
    inputs, ``scale`` included, stay indexed by input frame or group."""
    R = _branches(branches)
    if slots != 1 or delay != 0:                                # the link on the transmit groups, with the feedback groups' selection
        keys, ideal, est, sigma, rho, scale = (np.asarray(v) for v in (keys, ideal, est, sigma, rho, scale))
        if keys.ndim != 1 or any(v.shape[:1] != keys.shape for v in (ideal, est)) or sigma.size != keys.size or rho.size != keys.size:
            raise ValueError("keys, ideal, est, sigma and rho must hold one entry per frame")
        groups = _tx_grouped(len(keys), R)
        if scale.size != groups:
            raise ValueError(f"scale must hold one value per group ({groups}), got {scale.size}")
        sent, feedback = delayed_groups(groups, slots, delay)
        at, fb = _group_frames(sent, 2 * R), _group_frames(feedback, 2 * R)
        if pmi is None:
            pmi = precoding_pmi_host(cfg, est[fb], rho.reshape(-1)[fb], R, subband)
        return link_precoded_host(cfg, keys[at], ideal[at], est[at], sigma.reshape(-1)[at], rho.reshape(-1)[at], scale.reshape(-1)[sent], R,
                                  subband, factors, tau, e_lambda, pmi)
    index, n_sub = precoding_subbands(cfg, subband)
    keys, H, E, sigma = _checked(cfg, keys, ideal, est, sigma)
    n, (S, T) = len(keys), cfg.sim.ofdm
    G, W = _tx_grouped(n, R), 2 * R
    rho = _rho_of(rho, n)
    if np.size(scale) != G:
        raise ValueError(f"scale must hold one value per group ({G}), got {np.size(scale)}")
    if pmi is None:
        pmi = precoding_pmi_host(cfg, E, rho, R, subband)
    else:
        pmi = np.asarray(pmi)
        if pmi.shape != (G, n_sub) or pmi.dtype.kind not in "iu" or pmi.min() < 0 or pmi.max() > 3:
            raise ValueError(f"pmi must hold integers in 0 .. 3 of shape ({G}, {n_sub}), got {pmi.dtype} {pmi.shape}")
        pmi = pmi.astype(np.int32)
    at = pmi[:, index][:, :, None]                                               # [G, S, 1]: every subcarrier's index
    gi, gq, x = _sent(cfg, keys[::W])                                             # one transmission per group: the leader's key
    c = p = reach = p_reach = 0.0
    for r in range(R):                                                           # in increasing r, starting from 0
        sl = slice(2 * r, None, W)                                               # the frames (r, 0); (r, 1) follow them
        H0, H1, E0, E1 = H[sl], H[2 * r + 1::W], E[sl], E[2 * r + 1::W]
        noise = _noise(cfg, keys[sl], sigma[sl])
        y = (H0 * x + _mul_q(at, H1) * x) + noise                                # with H_r1 = 0: _branch's sample
        e = E0 + _mul_q(at, E1)
        ry, re = (np.abs(H0) + np.abs(H1)) * np.abs(x) + np.abs(noise), np.abs(E0) + np.abs(E1)
        w = rho[sl, None, None]
        c, p = c + w * (y * e.conj()), p + w * (e.real ** 2 + e.imag ** 2)
        reach, p_reach = reach + w * (ry * re), p_reach + w * (re * re)
    hard = _hard(cfg, gi, gq, c, p, reach, tau, p_reach)
    soft = _soft(cfg, gi, gq, c, p, reach, scale, factors, e_lambda, p_reach)
    return ((hard,) if tau is None else hard[:1]) + soft[:2] + (() if tau is None else hard[1:]) + soft[2:] + (pmi,)


# ---- the frame keys with torch ops, for frame numbers that live on the device (no synchronisation) ----

def _s64(v: int) -> int:
    v &= 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _lsr(x: torch.Tensor, k: int) -> torch.Tensor:
    return (x >> k) & ((1 << (64 - k)) - 1)


def _splitmix64_torch(x: torch.Tensor) -> torch.Tensor:
    """``synth._splitmix64`` on an int64 tensor taken as 64-bit words (two's-complement arithmetic wraps as the unsigned one does)."""
    x = x + _s64(0x9E3779B97F4A7C15)
    x = (x ^ _lsr(x, 30)) * _s64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _s64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def frame_keys_torch(seed: int, frame_ids: torch.Tensor) -> torch.Tensor:
    """``chansim.frame_keys`` for an integer tensor of frame numbers, on its device: int64 ``[n]`` holding the keys' bits."""
    sk = int(_splitmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64))[0])
    return _splitmix64_torch(frame_ids.reshape(-1).to(torch.int64) ^ _s64(sk))


class _FrameSweep:
    """What the accumulators of a sweep share: ``_measure`` turns a batch into what the accumulator asked ``_open`` for -- the counts, the
    loss or the LLRs of the link, with the diversity link's combiner in front when ``branches > 1``, the two-stream detector with
    ``streams=2`` or the Alamouti combiner with ``tx_diversity`` -- as tensors on the accumulator's device, whichever device that is.  ``_operands`` returns None for an empty batch, else ``(b, H, E, keys, per_frame)``: on a CPU
    device NumPy arrays for the float64 definition, on a HIP device tensors for the plan -- frame numbers and SNRs that are host
    tensors are hashed and converted on the host and copied from pinned memory, device tensors with torch ops, so nothing
    synchronises.  ``per_frame`` holds one float32 ``[b]`` operand per entry of ``of_snr``, pairs ``(numpy function, torch function on
    a float64 tensor)`` of the SNR in dB."""

    _runs_cwsic = False                            # detector="cwsic" needs the LDPC decoder between its detections: one subclass has it

    def _open(self, cfg: LinkConfig, device, seed: int, want: str, branches: int = 1, err_var: float = 0.0, factors=(1.0,),
              streams: int = 1, detector: str = "mmse", tx_diversity: Optional[str] = None,
              precoding_subband: Optional[int] = None, precoding_delay: int = 0, slots: int = 1) -> None:
        """``want``: which of ``"counts"``, ``"loss"`` and ``"llr"`` ``_measure`` computes.  ``streams=2``: the spatial-multiplexing
        link with ``detector`` in front (``streams=1`` ignores it).  ``tx_diversity``: None, or the pairing of the transmit-diversity
        link in front (one stream; ``detector`` is ignored).  ``precoding_subband``: None, or the subband width of the closed-loop
        link in front (one stream, no ``tx_diversity``; ``detector`` is ignored).  ``precoding_delay`` / ``slots``: the closed-loop link
        with feedback ``precoding_delay`` slots old on sequences of ``slots`` groups ("delayed feedback"); 0 is the instantaneous link,
        launch for launch, whatever ``slots``."""
        if not isinstance(cfg, LinkConfig):
            raise ValueError(f"{type(self).__name__} needs a LinkConfig (got {type(cfg).__name__})")
        self.cfg, self.seed, self._want = cfg, int(seed), want
        self.branches = _branches(branches)
        if isinstance(streams, bool) or not isinstance(streams, (int, np.integer)) or int(streams) not in (1, MAX_STREAMS):
            raise ValueError(f"streams = {streams!r}: 1, or {MAX_STREAMS} for the spatial-multiplexing link")
        self.streams, self.detector, self.tx_diversity = int(streams), detector, tx_diversity
        self._cwsic = isinstance(detector, str) and detector == CWSIC_DETECTOR
        if self._cwsic:                            # codeword cancellation decodes between its detections: one accumulator runs it
            if not self._runs_cwsic:
                _refuse_cwsic(detector, type(self).__name__, 'detector="sic" is the symbol-level cancellation this accumulator runs')
            if self.streams != MAX_STREAMS or tx_diversity is not None or precoding_subband is not None:
                raise ValueError(f'detector="cwsic" cancels one of {MAX_STREAMS} spatial streams: streams must be {MAX_STREAMS} (got '
                                 f"{self.streams}), tx_diversity None (got {tx_diversity!r}) and precoding_subband None (got "
                                 f'{precoding_subband!r}); one stream from two antennas has nothing to cancel -- use detector="mmse" there')
        if tx_diversity is not None:
            _pairing(tx_diversity)
            if self.streams != 1:
                raise ValueError(f"tx_diversity = {tx_diversity!r} sends one stream from two antennas: streams must be 1 (got {self.streams})")
        self.precoding_subband = None
        if precoding_subband is not None:
            if self.streams != 1 or tx_diversity is not None:
                raise ValueError(f"precoding_subband = {precoding_subband!r} sends one precoded stream from two antennas: streams must "
                                 f"be 1 (got {self.streams}) and tx_diversity None (got {tx_diversity!r})")
            self.precoding_subband = _subband(cfg, precoding_subband)
        if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in (precoding_delay, slots)) or precoding_delay < 0 \
                or slots < 1:
            raise ValueError(f"precoding_delay = {precoding_delay!r}, slots = {slots!r}: integers, the delay at least 0 and slots at least 1")
        self.precoding_delay, self.slots = int(precoding_delay), int(slots)
        if self.precoding_delay > 0:
            if self.precoding_subband is None:
                raise ValueError(f"precoding_delay = {precoding_delay} delays the PMI feedback of the closed-loop link: give "
                                 f"precoding_subband= as well (no other link has feedback to delay)")
            if self.slots <= self.precoding_delay:
                raise ValueError(f"precoding_delay = {precoding_delay} needs sequences longer than the delay: use slots >= "
                                 f"{self.precoding_delay + 1} (got slots = {slots}) on batches from ChannelSimConfig(slots=...)")
        self._pairs = tx_diversity is not None or self.precoding_subband is not None      # a group is 2 R frames and yields one row
        # frames per group: the branches, times the two transmit antennas or the streams
        self._width =self.branches * (2 if self._pairs else self.streams)
        if self.streams > 1:
            _sm_shape(0, self.branches, self.streams)           # one antenna cannot separate two streams
            _detector("mmse" if self._cwsic else detector)      # the detector's name: a linear one, "joint" or "sic"; "cwsic" starts as MMSE
        self.device = torch.device(device)
        soft = want != "counts"
        self._plan = None
        if self.device.type == "cuda":
            from . import hip_ops                  # loads the extension: a missing .so raises here, loudly
            if self.precoding_subband is not None:  # every measure of the closed-loop link comes from its one launch
                delayed = (self.slots, self.precoding_delay) if self.precoding_delay > 0 else ()
                self._plan = hip_ops.LinkPrecodedPlan(cfg, self.device, self.branches, self.precoding_subband, *delayed)
            elif tx_diversity is not None:         # every measure of the transmit-diversity link comes from the combiner's one launch
                self._plan = hip_ops.LinkAlamoutiPlan(cfg, self.device, self.branches, tx_diversity)
            elif self.streams > 1:                 # every measure of the spatial-multiplexing link comes from the detector's one launch
                plan = {JOINT_DETECTOR: hip_ops.LinkJointPlan, SIC_DETECTOR: hip_ops.LinkSicPlan}.get(detector, hip_ops.LinkSmPlan)
                self._plan = plan(cfg, self.device, self.branches, self.streams)
            elif self.branches == 1:
                self._plan = (hip_ops.LinkSoftPlan if soft else hip_ops.LinkPlan)(cfg, self.device)
            else:                                  # every measure of the diversity link comes from the combiner's one launch
                self._plan = hip_ops.LinkMrcPlan(cfg, self.device, self.branches)
            self.device = self._plan.device
        self.err_var = float(err_var)
        if not self.err_var >= 0.0:
            raise ValueError(f"err_var = {err_var!r}: a variance, at least 0")
        self.factors = _factors(factors)
        self._factors_t = None if self._plan is None else torch.from_numpy(self.factors).to(self.device)
        self._of_snr = (_SIGMA_OF_SNR, _SCALE_OF_SNR(self.err_var)) if soft or self._width > 1 else (_SIGMA_OF_SNR,)
        self.frames = 0
        if self.precoding_subband is not None:     # how often each precoder was chosen, summed on the device
            self._pmi_counts = torch.zeros(4, dtype=torch.int64, device=self.device)
            self._pmi_index = torch.arange(4, dtype=torch.int32, device=self.device)
        self._sic = self.streams > 1 and detector == SIC_DETECTOR
        if self._sic:                              # the launches' three integers, summed on the device
            self._sic_stats = torch.zeros(SIC_STATS, dtype=torch.int64, device=self.device)

    def _stage(self, a: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(a).pin_memory().to(self.device, non_blocking=True)

    def _operands(self, est, ideal, meta, frame_ids, snr_db, of_snr):
        S, T = self.cfg.sim.ofdm
        if ideal.dim() != 3 or tuple(ideal.shape[1:]) != (S, T) or ideal.dtype != torch.complex64:
            raise ValueError(f"ideal must be complex64 [B, {S}, {T}], got {ideal.dtype} {tuple(ideal.shape)}")
        if est is not None and (est.shape != ideal.shape or est.dtype != torch.complex64):
            raise ValueError(f"est must be complex64 {tuple(ideal.shape)} like ideal, got {est.dtype} {tuple(est.shape)}")
        b = ideal.shape[0]
        if frame_ids is None:
            if meta is None:
                raise ValueError("the frame numbers are needed: meta (file_no first) or frame_ids=")
            frame_ids = meta[0]
        if snr_db is None:
            if meta is None:
                raise ValueError("the SNR is needed: meta (snr second) or snr_db=")
            snr_db = meta[1]
        if b == 0:
            return None
        on_device = lambda v: torch.is_tensor(v) and v.device.type == "cuda"  # noqa: E731
        host = lambda v: v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)  # noqa: E731
        if self._plan is None or not on_device(frame_ids):
            g = np.rint(host(frame_ids).reshape(-1).astype(np.float64)).astype(np.int64)
            if g.size != b:
                raise ValueError(f"one frame number per frame ({b}), got {g.size}")
            keys = frame_keys(self.seed, g).view(np.int64)
        if self._plan is None or not on_device(snr_db):
            snr = host(snr_db).reshape(-1)
            if snr.size not in (1, b):
                raise ValueError(f"one SNR, or one per frame ({b}), got {snr.size}")
            per_frame = [on_host(np.broadcast_to(snr, (b,))) for on_host, _ in of_snr]
        if self._plan is None:
            H = ideal.detach().cpu().numpy()
            return b, H, (H if est is None else est.detach().cpu().numpy()), keys, per_frame
        dev = self.device
        if on_device(frame_ids):
            if frame_ids.numel() != b:
                raise ValueError(f"one frame number per frame ({b}), got {frame_ids.numel()}")
            ids = frame_ids.reshape(-1).to(dev)
            keys_t = frame_keys_torch(self.seed, ids if not ids.is_floating_point() else ids.round())
        else:
            keys_t = self._stage(keys)
        if on_device(snr_db):
            if snr_db.numel() not in (1, b):
                raise ValueError(f"one SNR, or one per frame ({b}), got {snr_db.numel()}")
            snr_t = snr_db.reshape(-1).to(device=dev, dtype=torch.float64)
            per_frame_t = [on_dev(snr_t).to(torch.float32).expand(b).contiguous() for _, on_dev in of_snr]
        else:
            per_frame_t = [self._stage(a) for a in per_frame]
        H = ideal.to(dev).contiguous()
        return b, H, (H if est is None else est.to(dev).contiguous()), keys_t, per_frame_t

    def _measure(self, est, ideal, meta, frame_ids, snr_db):
        """A batch of ``update``'s arguments: None for an empty one, else ``(groups, the leaders' keys, counts, loss, llr)`` on the
        accumulator's device, of which the one ``_open`` was asked for is there (the others may be None).  On a CPU device the float64
        definitions, which compute no soft output for counts alone; on a HIP device one launch -- ``aft_link_errors_f32`` for the
        counts and ``aft_link_soft_f32`` for the loss and the LLRs of a single branch, ``aft_link_mrc_f32`` for any of them with
        several, the weights formed by torch ops on the device -- and nothing synchronises.  With ``streams=2`` the groups are the
        ``G N`` stream-frames of the spatial-multiplexing link with the keys of frames ``(0, s)``: ``link_sm_host`` on a CPU device,
        one launch of ``aft_link_sm_f32`` with ``rho`` and ``reg`` formed on the device on a HIP device; with ``detector="joint"``
        ``link_joint_host`` and one launch of ``aft_link_joint_f32``, which has no ``reg``; with ``detector="sic"`` ``link_sic_host`` and
        one launch of ``aft_link_sic_f32`` with the MMSE ``reg``, and one add of the batch's three integers into the sums
        ``sic_propagation`` reads.  With ``tx_diversity`` the groups are the
        ``G`` transmissions of the transmit-diversity link with the leaders' keys: ``link_alamouti_host`` on a CPU device, one launch
        of ``aft_link_alamouti_f32`` with ``rho`` formed on the device on a HIP device.  With ``precoding_subband`` the same groups on
        the closed-loop link: ``link_precoded_host`` or one launch of ``aft_link_precoded_f32``, and one add of the batch's PMIs into
        the histogram ``pmi_histogram`` reads; with ``precoding_delay`` the batch is whole sequences of ``slots`` groups, the one launch
        is ``aft_link_precoded_delayed_f32``'s, and the groups returned are the transmitted ones, with the transmit slots' leader keys."""
        ops = self._operands(est, ideal, meta, frame_ids, snr_db, self._of_snr)
        if ops is None:
            return None
        b, H, E, keys, (sigma, *scale) = ops       # scale: the frames' LLR scales, where the measure or the combiner needs them
        G = _tx_grouped(b, self.branches) if self._pairs else _grouped(b, self.branches, self.streams)
        measure = self._measure_host if self._plan is None else self._measure_device
        if self.precoding_delay > 0:               # whole sequences; the warm-up slots of each yield no row
            if G % self.slots:
                raise ValueError(f"a batch of {b} frames is not a multiple of slots * 2 * branches = {self.slots} * 2 * {self.branches}")
            return (G // self.slots * (self.slots - self.precoding_delay), *measure(G, H, E, keys, sigma, scale))
        return (G * self.streams, *measure(G, H, E, keys, sigma, scale))

    def _measure_host(self, G, H, E, keys, sigma, scale):
        """The float64 definitions on NumPy operands: ``(the leaders' keys, counts, loss, llr)`` as host tensors."""
        R, N = self.branches, self.streams
        counts = loss = llr = None
        if self.precoding_subband is not None:     # G precoded transmissions from two antennas, with the leaders' keys
            delayed = dict(slots=self.slots, delay=self.precoding_delay) if self.precoding_delay > 0 else {}
            counts, loss, llr, pmi = link_precoded_host(self.cfg, keys, H, E, sigma, *_weights(scale[0], 2 * R), R,
                                                        self.precoding_subband, self.factors, **delayed)
            self._count_pmi(torch.from_numpy(pmi))
            sent = keys[::2 * R]
            if delayed:                            # the leaders of the transmit slots
                sent = np.ascontiguousarray(sent[delayed_groups(G, self.slots, self.precoding_delay)[0]])
        elif self.tx_diversity is not None:        # G transmissions from two antennas, with the leaders' keys
            counts, loss, llr = link_alamouti_host(self.cfg, keys, H, E, sigma, *_weights(scale[0], 2 * R), R, self.tx_diversity,
                                                   self.factors)
            sent = keys[::2 * R]
        elif N > 1:                                # G N "frames": stream s of group g, with the key of frame (0, s)
            rho, lead = _weights(scale[0], R * N)
            if self.detector == JOINT_DETECTOR:
                out = link_joint_host(self.cfg, keys, H, E, sigma, rho, lead, R, N, self.factors)
            elif self._sic:                        # MMSE-SIC: the first stage is the MMSE detector
                *out, stats = link_sic_host(self.cfg, keys, H, E, sigma, rho, lead, detector_reg(lead, "mmse"), R, N, self.factors)
                self._sic_stats += torch.from_numpy(stats.sum(axis=0))
            else:
                out = link_sm_host(self.cfg, keys, H, E, sigma, rho, lead, detector_reg(lead, self.detector), R, N, self.factors)
            counts, loss, llr = (v.reshape(G * N, *v.shape[2:]) for v in out)
            sent = np.ascontiguousarray(keys.reshape(G, R, N)[:, 0, :]).reshape(-1)
        else:
            sent = keys[::R]
            if R > 1:
                counts, loss, llr = link_mrc_host(self.cfg, keys, H, E, sigma, *_weights(scale[0], R), R, self.factors)
            elif self._want == "counts":
                counts = link_errors_host(self.cfg, keys, H, E, sigma)
            else:
                loss, llr = link_llrs_host(self.cfg, keys, H, E, sigma, scale[0], self.factors)
        return tuple(None if a is None else torch.from_numpy(a) for a in (sent, counts, loss, llr))

    @staticmethod
    def _device_weights(scale: torch.Tensor, width: int):
        """``_weights`` by torch ops on the device: ``(rho [b], the leaders' scale [b / width])`` of groups of ``width`` frames."""
        s = scale.view(-1, width).to(torch.float64)
        return (s / s[:, :1]).to(torch.float32).reshape(-1), scale[::width].contiguous()

    def _measure_device(self, G, H, E, keys, sigma, scale):
        """The plan's one launch on device operands: ``(the leaders' keys, counts, loss, llr)`` on the device."""
        R, N, want_llr = self.branches, self.streams, self._want == "llr"
        counts = loss = llr = None
        if self._pairs:                            # the weights of the frames (r, 0) against the leader's, over the 2 R frames of a group
            rho, lead = self._device_weights(scale[0], 2 * R)
            counts, loss, llr, *pmi = self._launch(H, E, keys, sigma, rho, lead, self._factors_t, want_llr=want_llr)
            if pmi:                                # the closed-loop link's fourth output
                self._count_pmi(pmi[0])
            if self.precoding_delay > 0:           # the leaders of the transmit slots: a strided view, then one copy
                return keys[::2 * R].view(-1, self.slots)[:, self.precoding_delay:].reshape(-1), counts, loss, llr
            return keys[::2 * R].contiguous(), counts, loss, llr
        if N > 1:                                  # the detectors differ in one operand: the joint one has no regulariser
            rho, lead = self._device_weights(scale[0], R * N)
            if self.detector == JOINT_DETECTOR:
                reg = ()
            else:
                reg = (torch.zeros_like(lead) if self.detector == "zf" else (1.0 / lead.to(torch.float64)).to(torch.float32),)   # "sic": MMSE's
            counts, loss, llr, *stats = self._launch(H, E, keys, sigma, rho, lead, *reg, self._factors_t, want_llr=want_llr)
            if stats:                              # the successive-cancellation link's fourth output: one sum, one add
                self._sic_stats += stats[0].sum(dim=0, dtype=torch.int64)
            return keys.view(G, R, N)[:, 0, :].reshape(-1), counts, loss, llr
        if R > 1:
            rho, lead = self._device_weights(scale[0], R)
            counts, loss, llr = self._launch(H, E, keys, sigma, rho, lead, self._factors_t, want_llr=want_llr)
        elif self._want == "counts":
            counts = self._launch(H, E, keys, sigma)
        else:
            loss, llr = self._launch(H, E, keys, sigma, scale[0], self._factors_t, want_llr=want_llr)
        return keys[::R].contiguous(), counts, loss, llr

    def _count_pmi(self, pmi: torch.Tensor) -> None:
        """A batch's PMIs ``[G, n_sub]`` into the histogram: one comparison against 0 .. 3, one sum, one add; nothing synchronises."""
        self._pmi_counts += (pmi.reshape(-1, 1) == self._pmi_index).sum(dim=0)

    def pmi_histogram(self, group=None) -> list:
        """How often each of the four precoders was chosen over the sweep, all ranks: four integers; one read, as the result's."""
        if self.precoding_subband is None:
            raise ValueError("pmi_histogram needs precoding_subband: no other link chooses a precoder")
        return [int(v) for v in self._all_ranks(self._pmi_counts.to(torch.float64), group)]

    def sic_propagation(self, group=None) -> tuple:
        """What successive cancellation did over the sweep, all ranks: ``(the share of data elements detected in swapped order -- stream
        1 first --, the symbol-error rate of the first decision, the share of first-decision errors followed by a symbol error of the
        other stream)``; 0.0 where a denominator is 0.  Summed on the device by one add per batch; one read, as the result's."""
        if not self._sic:
            raise ValueError('sic_propagation needs streams=2 and detector="sic": no other link cancels a decided stream')
        elements = torch.tensor([self.frames // self.streams * self.cfg.data_elements], dtype=torch.float64, device=self.device)
        swapped, wrong, both, elements = self._all_ranks(torch.cat([self._sic_stats.to(torch.float64), elements]), group)
        return (swapped / elements if elements > 0 else 0.0, wrong / elements if elements > 0 else 0.0, both / wrong if wrong > 0 else 0.0)

    @staticmethod
    def _total(per_group: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
        """A batch's sum over its groups, as ``dtype``.  Host tensors are summed by NumPy, which adds the groups in index order: float64
        losses then add up as a caller of the definition adds them, bit for bit."""
        if per_group.is_cuda:
            return per_group.sum(dim=0, dtype=dtype)
        return torch.from_numpy(per_group.numpy().sum(axis=0)).to(dtype)

    def _launch(self, *args, plan=None, **kw):
        """The plan (``self._plan`` unless another is given) on the accumulator's device: the launch belongs to it, whichever device
        is current."""
        plan = self._plan if plan is None else plan
        if torch.cuda.current_device() != self.device.index:
            with torch.cuda.device(self.device):
                return plan(*args, **kw)
        return plan(*args, **kw)

    @staticmethod
    def _all_ranks(local: torch.Tensor, group) -> list:
        """The sweep's one read: ``local`` (float64, on the device) summed over all ranks -- with several, one all-gather."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():   # world_size 1 included: same code path on every launch
            gathered = [torch.empty_like(local) for _ in range(dist.get_world_size(group))]
            dist.all_gather(gathered, local, group=group)
            local = torch.stack(gathered).sum(dim=0)
        return local.tolist()


_SIGMA_OF_SNR = (noise_sigma, lambda snr: torch.pow(10.0, -snr / 20.0))
_SCALE_OF_SNR = lambda err_var: (lambda snr: llr_scale(snr, err_var), lambda snr: 1.0 / (torch.pow(10.0, -snr / 10.0) + err_var))  # noqa: E731


class LinkAccumulator(_FrameSweep):
    """Bit and symbol errors of a sweep, with the surface of ``metrics.MseAccumulator``: ``update`` per batch, ``result`` once.

    ``update(est, ideal, meta)`` takes the frames' numbers from ``meta[0]`` (the loaders' ``file_no``: float32 as the reference's, so
    exact below 2^24; ``frame_ids=`` gives exact ones) and their SNR from ``meta[1]`` (``snr_db=`` overrides; one value or one per
    frame); the frame's key is ``chansim.frame_keys(seed, g)``.  ``est=None`` is perfect channel knowledge (``est = ideal``).  On a HIP
    device a batch is one launch of ``aft_link_errors_f32`` plus one small integer add into an int64 ``[2]`` device tensor: frame
    numbers and SNRs that are host tensors are hashed on the host and copied from pinned memory, device tensors are hashed with
    torch ops -- nothing synchronises.  On a CPU device the float64 definition runs.  ``result`` / ``result_ser`` close the sweep with
    one read and, with several ranks, the same 16-byte all-gather as the MSE accumulator.

    ``branches=R`` (module docstring, "the diversity link"; the same argument on the three accumulators below): every R consecutive
    frames of a batch are the branches of one receiver, combined by one launch of ``aft_link_mrc_f32`` (on a CPU device by
    ``link_mrc_host``) with the weights of ``branch_weights``; a batch that is no multiple of R raises ``ValueError``, ``frames``
    counts the groups, and every rate is per transmission.  ``branches=1`` is the single-branch path, launch for launch.

    ``streams=2`` with ``detector`` ``"zf"`` or ``"mmse"`` (module docstring, "the spatial-multiplexing link"; the same arguments on
    ``RateAccumulator``, ``BlockErrorAccumulator`` and ``LdpcBlockErrorAccumulator``, not on ``HarqAccumulator``): every ``2 R``
    consecutive frames of a batch are the (antenna, stream) pairs of one receiver, ``R >= 2``, detected by one launch of
    ``aft_link_sm_f32`` (on a CPU device by ``link_sm_host``) with ``rho`` and ``reg`` formed on the device without a synchronisation;
    a batch that is no multiple of ``2 R`` raises ``ValueError``.  A batch yields ``G N`` "frames", stream ``s`` of group ``g`` with the
    key of frame ``(0, s)``; ``frames`` counts them, and every rate is per stream and symbol: the spectral efficiency is N times it.
    ``detector="joint"`` (module docstring, "the joint link") is the joint max-log demapper on the same frames: one launch of
    ``aft_link_joint_f32`` (on a CPU device ``link_joint_host``), no regulariser.
    ``detector="sic"`` (module docstring, "the successive-cancellation link") is ordered MMSE-SIC on the same frames: one launch of
    ``aft_link_sic_f32`` (on a CPU device ``link_sic_host``) with the MMSE regulariser; ``sic_propagation()`` reads what it propagated.
    ``streams=1`` is today's path, launch for launch, and ignores ``detector``.

    ``tx_diversity="time"`` or ``"frequency"`` (module docstring, "the transmit-diversity link"; the same keyword on ``RateAccumulator``,
    ``BlockErrorAccumulator`` and ``LdpcBlockErrorAccumulator``, not on ``HarqAccumulator``): every ``2 R`` consecutive frames of a batch
    are the (receive antenna, transmit antenna) pairs of one receiver, ``R = branches`` in 1 .. 8, and the two transmit antennas send
    ONE stream as Alamouti pairs over adjacent data symbols or subcarriers, combined by one launch of ``aft_link_alamouti_f32`` (on a
    CPU device by ``link_alamouti_host``) with ``rho`` formed on the device without a synchronisation.  ``streams`` must be 1
    (``ValueError`` otherwise), ``detector`` is ignored, a batch that is no multiple of ``2 R`` raises ``ValueError``; a batch yields
    ``G`` rows with the leaders' keys and ``frames`` counts them.  The SNR is per transmit antenna.  ``tx_diversity=None`` is today's
    path, launch for launch.

    ``precoding_subband=B`` (module docstring, "the closed-loop link"; the same keyword on the same four accumulators): the same
    ``2 R`` frames per group, the two transmit antennas sending ONE stream co-phased by a codebook precoder that the receiver picks
    per subband of ``B`` subcarriers from the estimate, by one launch of ``aft_link_precoded_f32`` (on a CPU device by
    ``link_precoded_host``).  ``streams`` must be 1 and ``tx_diversity`` None (``ValueError`` otherwise), ``detector`` is ignored; rows,
    keys, ``frames`` and the SNR as under ``tx_diversity``.  ``pmi_histogram()`` reads how often each of the four precoders was
    chosen, summed on the device by one add per batch.  ``precoding_subband=None`` is today's path, launch for launch.

    ``precoding_delay=d`` with ``slots=K`` (module docstring, "delayed feedback"; the same keywords on the same four accumulators,
    not on ``HarqAccumulator``): every ``K`` consecutive groups of a batch are the slots of one sequence -- batches of
    ``ChannelSimConfig(slots=K, antennas=(R, 2))`` --, slot ``k >= d`` is sent with the PMIs selected ``d`` slots earlier and the first
    ``d`` slots of a sequence are warm-up: one launch of ``aft_link_precoded_delayed_f32`` (on a CPU device ``link_precoded_host`` with
    ``slots`` and ``delay``).  ``frames`` and every rate count the transmitted groups only, ``pmi_histogram()`` the APPLIED precoders.
    Needs ``precoding_subband`` and ``slots > d`` (``ValueError`` otherwise); a batch that is no multiple of ``K 2 R`` frames raises
    ``ValueError``.  ``precoding_delay=0`` is the instantaneous path, launch for launch, whatever ``slots``."""

    def __init__(self, cfg: LinkConfig, device, seed: int = 0, branches: int = 1, streams: int = 1, detector: str = "mmse", *,
                 tx_diversity: Optional[str] = None, precoding_subband: Optional[int] = None, precoding_delay: int = 0,
                 slots: int = 1) -> None:
        self._open(cfg, device, seed, "counts", branches, streams=streams, detector=detector, tx_diversity=tx_diversity,
                   precoding_subband=precoding_subband, precoding_delay=precoding_delay, slots=slots)
        self.errors = torch.zeros(2, dtype=torch.int64, device=self.device)     # bit errors, symbol errors

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        got = self._measure(est, ideal, meta, frame_ids, snr_db)
        if got is not None:
            groups, _, counts, _, _ = got
            self.errors += self._total(counts, torch.int64)
            self.frames += groups

    def local_pair(self, which: int = 0) -> torch.Tensor:
        """float64 ``[2]`` on the device: (bit errors, bits sent) -- with ``which=1`` (symbol errors, symbols sent).  Exact below 2^53."""
        sent = self.frames * (self.cfg.bits_per_frame if which == 0 else self.cfg.data_elements)
        return torch.stack([self.errors[which].to(torch.float64), torch.tensor(float(sent), dtype=torch.float64, device=self.device)])

    def _rate(self, which: int, group) -> float:
        errors, sent = self._all_ranks(self.local_pair(which), group)
        return errors / sent if sent > 0 else 0.0

    def result(self, group: Optional["torch.distributed.ProcessGroup"] = None) -> float:
        """Global bit-error rate over all ranks (integers summed: identical on every rank, whatever the order)."""
        return self._rate(0, group)

    def result_ser(self, group=None) -> float:
        """Global symbol-error rate."""
        return self._rate(1, group)


class RateAccumulator(_FrameSweep):
    """The achievable rate of a sweep from its max-log LLRs (module docstring, "the soft link"), with ``LinkAccumulator``'s ``update``
    surface.  A frame's LLR scale is ``llr_scale(snr_db, err_var)``: ``err_var`` is what the caller knows of the estimate's error
    variance (0: the LLRs trust the estimate as if it were the channel), and ``factors`` the grid of further scale factors the loss is
    evaluated on in the same pass.  On a HIP device a batch is one launch of ``aft_link_soft_f32`` plus one float64 add into a device
    tensor ``[K]``; nothing synchronises.  On a CPU device the float64 definition runs.  ``result`` returns the K rates in bit/symbol
    (``m - loss / data elements``; a rate may be negative), ``result_gmi`` their maximum; either is one read and, with several ranks,
    one all-gather of ``K + 1`` float64 (the K losses and the frames).  The losses are float sums: ranks that split a sweep differently
    agree to rounding, not bit for bit -- every rank of one sweep reports the same number.  ``branches``, ``streams``, ``detector`` and
    ``tx_diversity`` as ``LinkAccumulator``'s: with ``tx_diversity`` the rate is per transmission of the two antennas."""

    def __init__(self, cfg: LinkConfig, device, seed: int = 0, factors=(1.0,), err_var: float = 0.0, branches: int = 1,
                 streams: int = 1, detector: str = "mmse", *, tx_diversity: Optional[str] = None,
                 precoding_subband: Optional[int] = None, precoding_delay: int = 0, slots: int = 1) -> None:
        self._open(cfg, device, seed, "loss", branches, err_var, factors, streams, detector, tx_diversity, precoding_subband,
                   precoding_delay, slots)
        self.loss = torch.zeros(len(self.factors), dtype=torch.float64, device=self.device)

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        got = self._measure(est, ideal, meta, frame_ids, snr_db)
        if got is not None:
            groups, _, _, loss, _ = got
            self.loss += self._total(loss, torch.float64)
            self.frames += groups

    def result(self, group: Optional["torch.distributed.ProcessGroup"] = None) -> list:
        """The K rates in bit/symbol over all ranks, one per factor (0.0 each for an empty sweep)."""
        frames = torch.tensor([float(self.frames)], dtype=torch.float64, device=self.device)
        *loss, frames = self._all_ranks(torch.cat([self.loss, frames]), group)
        m, elements = self.cfg.bits_per_symbol, frames * self.cfg.data_elements
        return [m - v / elements if elements > 0 else 0.0 for v in loss]

    def result_gmi(self, group=None) -> float:
        """The best rate of the factor grid: the GMI's supremum over the LLR scale, taken on the grid."""
        return max(self.result(group))


_REFINE_LINKS = ("refine= runs on the single-stream link -- one transmit antenna, branches=R receive antennas (get_link_stats, "
                 "get_link_rates, get_link_bler and get_link_harq with branches=) --")


class DataAidedRefiner(_FrameSweep):
    """Decision-directed refinement of a channel estimate (module docstring, "the decision-directed observation"; ``lmmse``: "the
    full-grid smoother"): a receiver that demodulates with ``est``, divides every received data sample by its own hard decision, and
    re-estimates the channel from ALL grid positions.  ``refine(est, pilots, ideal, meta)`` -> ``est'`` complex64 like ``est``; each of
    the ``iterations`` passes is observe (``link_observe_host`` / ``aft_link_observe_f32``) then smooth (``lmmse_grid_host`` /
    ``aft_lmmse_grid_f32`` with ``noise_scale = data_noise_scale(m)``), and pass ``i + 1`` decides with pass ``i``'s estimate.  The
    frames' keys and noise scales are the ones ``LinkAccumulator(link_cfg, device, seed, branches)`` forms from the same ``meta`` /
    ``frame_ids`` / ``snr_db``, so the refiner sees the very received samples the accumulator then measures ``est'`` on; the design
    point of the smoother is each frame's own ``meta`` (``assume`` pins conditions, as ``LmmseEstimator``'s).  ``branches=R``: the R
    frames of a group are decided together, with the combiner weights ``branch_weights(snr_db, err_var, R)`` -- give the ``err_var`` of
    the accumulator that measures the result (the coded ones take one), or the two combine with different weights --, and each is
    re-estimated from its own samples.  ``source="sent"`` divides by the sent
    symbols instead: the genie bound.  ``iterations=0`` returns ``est`` itself.  On a HIP device a pass is two launches on the current
    stream and nothing synchronises (the group weights are formed once per batch by torch ops); on a CPU device the float64 twins
    run.  ``symbol_error_rate()`` reads, once, the rate of wrong decisions of the LAST pass over everything refined so far."""

    def __init__(self, link_cfg: LinkConfig, device, seed: int = 0, branches: int = 1, iterations: int = 1, source: str = "decided",
                 assume=None, err_var: float = 0.0) -> None:
        from .lmmse import LmmseTables, _check_assume
        if not isinstance(link_cfg, LinkConfig):
            raise ValueError(f"DataAidedRefiner needs a LinkConfig (got {type(link_cfg).__name__})")
        if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
            raise ValueError(f"iterations = {iterations!r}: an integer, at least 0")
        self.cfg, self.seed, self.branches, self.iterations = link_cfg, int(seed), _branches(branches), int(iterations)
        self.source = source
        _source(source)
        self.assume = _check_assume(assume)
        self.tables = LmmseTables(link_cfg.sim)
        self.tables.grid()                                      # refuses a grid the smoother does not cover, here and not mid-sweep
        self.noise_scale = data_noise_scale(link_cfg.bits_per_symbol)
        self.device = torch.device(device)
        self._plan = self._smooth = None
        if self.device.type == "cuda":
            from . import hip_ops                               # loads the extension: a missing .so raises here, loudly
            self._plan = hip_ops.LinkObservePlan(link_cfg, self.device, self.branches, source)
            self.device = self._plan.device
            self._smooth = hip_ops.LmmseGridPlan(self.tables, self.device, assume=self.assume, noise_scale=self.noise_scale)
        self.err_var = float(err_var)
        if not self.err_var >= 0.0:
            raise ValueError(f"err_var = {err_var!r}: a variance, at least 0")
        self._of_snr = (_SIGMA_OF_SNR, _SCALE_OF_SNR(self.err_var))
        self.errors = torch.zeros((), dtype=torch.int64, device=self.device)     # wrong decisions of the last pass, summed on the device
        self.groups = 0

    def _conditions(self, meta, snr_db, b):
        """The smoother's per-frame conditions: None where ``assume`` pins, else ``meta``'s (``snr_db=`` overrides the SNR)."""
        fixed = self.tables.fixed(self.assume)
        given = [snr_db if snr_db is not None else (None if meta is None else meta[1])] + \
                [None if meta is None else meta[k] for k in (2, 3)]
        out = []
        for name, v, f in zip(("snr_db", "delay_spread_ns", "doppler_hz"), given, fixed):
            if f >= 0:
                out.append(None)
                continue
            if v is None:
                raise ValueError(f"the smoother needs each frame's {name}: meta, or assume= to pin it")
            v = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float32))
            v = v.reshape(-1).to(torch.float32)
            if v.numel() == 1:
                v = v.expand(b)
            if v.numel() != b:
                raise ValueError(f"one {name} per frame ({b}), got {v.numel()}")
            out.append(v.contiguous())
        return out

    def refine(self, est: torch.Tensor, pilots: torch.Tensor, ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> torch.Tensor:
        if est is None:
            raise ValueError("refine needs an estimate to start from: est=None is perfect channel knowledge, which nothing refines")
        Ps, Pt = self.cfg.sim.pilot
        if pilots.dim() != 3 or tuple(pilots.shape[1:]) != (Ps, Pt) or pilots.shape[0] != ideal.shape[0] or pilots.dtype != torch.complex64:
            raise ValueError(f"pilots must be complex64 [{ideal.shape[0]}, {Ps}, {Pt}], got {pilots.dtype} {tuple(pilots.shape)}")
        if self.iterations == 0:
            return est
        ops = self._operands(est, ideal, meta, frame_ids, snr_db, self._of_snr)
        if ops is None:
            return est
        b, H, E, keys, (sigma, scale) = ops
        G = _grouped(b, self.branches)
        conds = self._conditions(meta, snr_db, b)
        if self._plan is None:
            from .lmmse import lmmse_grid_host                  # lmmse imports nothing from this module at load time
            rho = _weights(scale, self.branches)[0]
            cond = np.zeros((b, 3))
            for k, c in enumerate(conds):
                if c is not None:
                    cond[:, k] = c.detach().cpu().double().numpy()
            P = pilots.detach().cpu().numpy()
            for _ in range(self.iterations):
                z, _, errors = link_observe_host(self.cfg, keys, H, E, sigma, rho, P, self.branches, self.source)
                E = lmmse_grid_host(self.tables, z, cond, self.assume, self.noise_scale).astype(np.complex64)
            self.errors += int(errors.sum())
            self.groups += G
            return torch.from_numpy(E)
        rho = self._device_weights(scale, self.branches)[0]
        P = pilots.to(self.device).contiguous()
        conds = [None if c is None else (c.pin_memory() if c.device.type == "cpu" else c).to(self.device, non_blocking=True) for c in conds]
        for _ in range(self.iterations):
            z, _, errors = self._launch(H, E, keys, sigma, rho, P)
            E = self._launch(z, *conds, plan=self._smooth)
        self.errors += errors.sum(dtype=torch.int64)
        self.groups += G
        return E

    def symbol_error_rate(self, group=None) -> float:
        """The share of data elements the LAST pass decided wrongly, over everything refined so far and all ranks; one read."""
        sent = torch.tensor(float(self.groups * self.cfg.data_elements), dtype=torch.float64, device=self.device)
        errors, sent = self._all_ranks(torch.stack([self.errors.to(torch.float64), sent]), group)
        return errors / sent if sent > 0 else 0.0


def as_refiner(refine, link_cfg: LinkConfig, device, seed: int = 0, branches: int = 1, streams: int = 1,
               tx_diversity: Optional[str] = None, precoding_subband: Optional[int] = None,
               err_var: float = 0.0) -> Optional[DataAidedRefiner]:
    """What the sweeps' ``refine=`` means: None -> None; an iteration count -> ``DataAidedRefiner(link_cfg, device, seed, branches,
    iterations, err_var=err_var)``; a ``DataAidedRefiner`` -> itself, provided it was built for this link, seed, branches and -- with
    several branches, where it sets the combiner's weights -- ``err_var``.  Two streams, transmit
    diversity and precoding are refused: their received samples mix two channels, which this observation does not separate."""
    if refine is None:
        return None
    if streams != 1 or tx_diversity is not None or precoding_subband is not None:
        raise ValueError(f"{_REFINE_LINKS} not with streams = {streams!r}, tx_diversity = {tx_diversity!r}, precoding_subband = "
                         f"{precoding_subband!r}: a received sample there mixes two channels")
    if isinstance(refine, DataAidedRefiner):
        if refine.cfg != link_cfg or refine.seed != int(seed) or refine.branches != branches or \
                (branches > 1 and refine.err_var != float(err_var)):
            raise ValueError("the refiner was built for another link, seed, number of branches or err_var than the sweep it is given to: it "
                             "would refine on other received samples, or combine them with other weights, than the sweep measures")
        return refine
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)) or refine < 0:
        raise ValueError(f"refine = {refine!r}: None, an iteration count (0, 1, 2, ...) or a DataAidedRefiner")
    if device is None:                                          # asked for the checks alone
        return None
    return DataAidedRefiner(link_cfg, device, seed, branches, int(refine), err_var=err_var)


# ---- the coded link (module docstring, "the coded link"): integer NumPy, mirrored by csrc/k_linkcode.hip ----

CODE_TAIL = 6                                               # constraint length 7
MAX_INFO_BITS = _abi.AFT_LINK_CODE_MAX_INFO_BITS
GOLDEN_STRIDE = 0.3819660112501051                          # 2 - the golden ratio
#: rate -> (the library's constant, which of (A, B) each step of the period keeps)
RATES = {"1/2": (_abi.AFT_LINK_RATE_1_2, ((1, 1),)),
         "2/3": (_abi.AFT_LINK_RATE_2_3, ((1, 1), (1, 0))),
         "3/4": (_abi.AFT_LINK_RATE_3_4, ((1, 1), (1, 0), (0, 1)))}
_GEN_A, _GEN_B = 0o133, 0o171                                # on the window u_t .. u_{t-6}, u_t the top bit
_PARITY = np.array([bin(i).count("1") & 1 for i in range(128)], dtype=np.int32)


def keep_mask(info_bits: int, rate: str) -> np.ndarray:
    """bool ``[K + 6, 2]``: which of (A_t, B_t) the puncturing keeps."""
    pattern = np.array(RATES[rate][1], dtype=bool)
    return pattern[np.arange(int(info_bits) + CODE_TAIL) % len(pattern)]


def coded_bits(info_bits: int, rate: str) -> int:
    """``n``: the kept outputs of the ``K + 6`` steps of a block."""
    return int(keep_mask(info_bits, rate).sum())


def default_stride(used_bits: int) -> int:
    """The smallest integer at least ``max(1, floor(0.3819660112501051 U))`` that is coprime to ``U``."""
    a = max(1, int(math.floor(GOLDEN_STRIDE * used_bits)))
    while math.gcd(a, used_bits) != 1:
        a += 1
    return a


def conv_encode(u, rate: str = "1/2") -> np.ndarray:
    """The zero-terminated, punctured codewords uint8 ``[..., n]`` of the inputs ``u`` ``[..., K]`` (0 / 1)."""
    u = np.asarray(u).astype(np.uint8)
    K = u.shape[-1]
    pad = np.zeros((*u.shape[:-1], CODE_TAIL), dtype=np.uint8)
    x = np.concatenate([pad, u, pad], axis=-1)               # x[t + 6 - i] = u_{t-i}
    d = lambda i: x[..., CODE_TAIL - i:CODE_TAIL - i + K + CODE_TAIL]  # noqa: E731
    a = d(0) ^ d(2) ^ d(3) ^ d(5) ^ d(6)
    b = d(0) ^ d(1) ^ d(2) ^ d(3) ^ d(6)
    return np.stack([a, b], axis=-1)[..., keep_mask(K, rate)]


@dataclass(frozen=True)
class CodeConfig:
    """A convolutional code on a link: ``info_bits`` = K per block, ``rate`` one of ``RATES``, the interleaver's ``stride`` (None: the
    golden-section default) and the quantiser's gain.  Derives ``coded_bits`` n, ``blocks`` B, ``used_bits`` U, ``stride_inverse`` and
    ``info_bits_per_frame``; refuses what ``aft_link_decode_f32`` refuses."""
    link: LinkConfig = field(default_factory=LinkConfig)
    info_bits: int = 1024
    rate: str = "1/2"
    stride: Optional[int] = None
    qgain: float = 8.0

    def __post_init__(self) -> None:
        if not isinstance(self.link, LinkConfig):
            raise ValueError(f"CodeConfig needs a LinkConfig (got {type(self.link).__name__})")
        K = self.info_bits
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= int(K) <= MAX_INFO_BITS:
            raise ValueError(f"info_bits = {K!r}: an integer in 1 .. {MAX_INFO_BITS}")
        object.__setattr__(self, "info_bits", int(K))
        if self.rate not in RATES:
            raise ValueError(f"rate = {self.rate!r}: one of {tuple(RATES)}")
        if self.blocks == 0:
            raise ValueError(f"a frame carries {self.link.bits_per_frame} bits, fewer than the {self.coded_bits} coded bits of one block")
        if self.info_bits_per_frame > 1 << 31:
            raise ValueError(f"{self.blocks} blocks of {self.info_bits} information bits: more than 2^31, where the hash's index and the "
                             f"int32 counts end")
        U = self.used_bits
        a = default_stride(U) if self.stride is None else self.stride
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 1 <= int(a) < U:
            raise ValueError(f"stride = {a!r}: an integer in [1, {U})")
        if math.gcd(int(a), U) != 1:
            raise ValueError(f"stride = {a} is not coprime to the {U} used bits")
        object.__setattr__(self, "stride", int(a))
        with np.errstate(over="ignore", under="ignore"):
            g = np.float32(self.qgain)
        if not (np.isfinite(g) and g > 0):
            raise ValueError(f"qgain = {self.qgain!r}: a finite positive float32")
        object.__setattr__(self, "qgain", float(g))

    @property
    def rate_code(self) -> int:
        return RATES[self.rate][0]

    @property
    def steps(self) -> int:
        return self.info_bits + CODE_TAIL

    @property
    def coded_bits(self) -> int:
        return coded_bits(self.info_bits, self.rate)

    @property
    def blocks(self) -> int:
        return self.link.bits_per_frame // self.coded_bits

    @property
    def used_bits(self) -> int:
        return self.blocks * self.coded_bits

    @property
    def stride_inverse(self) -> int:
        return pow(self.stride, -1, self.used_bits)

    @property
    def info_bits_per_frame(self) -> int:
        return self.blocks * self.info_bits

    def positions(self) -> np.ndarray:
        """int64 ``[B, n]``: the data-bit index ``j = (p stride) mod U`` of coded bit ``i`` of block ``b``, ``p = b n + i``."""
        U, p = self.used_bits, np.arange(self.used_bits, dtype=np.int64)
        if U <= 1 << 31:
            j = (p * np.int64(self.stride)) % np.int64(U)
        else:
            j = np.array([(int(v) * self.stride) % U for v in p], dtype=np.int64)
        return j.reshape(self.blocks, self.coded_bits)


def _keys64(keys) -> np.ndarray:
    keys = np.ascontiguousarray(keys)
    if keys.dtype == np.int64:
        keys = keys.view(np.uint64)
    if keys.dtype != np.uint64 or keys.ndim != 1:
        raise ValueError("keys must be a vector of 64-bit words (uint64, or int64 taken bit for bit)")
    return keys


def link_encode_host(code: CodeConfig, keys) -> Tuple[np.ndarray, np.ndarray]:
    """The information bits uint8 ``[n, B, K]`` and the codewords uint8 ``[n, B, coded_bits]`` of the frames with ``keys``."""
    keys = _keys64(keys)
    B, K = code.blocks, code.info_bits
    index = np.arange(B * K, dtype=np.uint64).reshape(1, B, K)
    info = (words(keys[:, None, None], STREAM_CODE_BITS, index) >> np.uint64(63)).astype(np.uint8)
    return info, conv_encode(info, code.rate)


def quantise(lam, qgain: float) -> np.ndarray:
    """``clamp(rint(float32(lam qgain)), -127, 127)`` as int32: one float32 product, ties to even, NaN gives 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(lam, dtype=np.float32) * np.float32(qgain)
        z = np.clip(np.rint(v), -127.0, 127.0)
    return np.where(np.isnan(v), np.float32(0), z).astype(np.int32)


def viterbi_host(z: np.ndarray) -> np.ndarray:
    """The decoder of the definition on depunctured int32 inputs ``z [..., steps, 2]`` (0 where punctured): the inputs uint8
    ``[..., steps]`` on the surviving path to state 0 (the last six are the tail's zeros)."""
    z = np.asarray(z, dtype=np.int32)
    lead, steps = z.shape[:-2], z.shape[-2]
    z = z.reshape(-1, steps, 2)
    R = z.shape[0]
    n = np.arange(64)
    pred = np.stack([(n & 31) << 1, ((n & 31) << 1) | 1])                       # [2, 64]
    window = ((n >> 5) << 6) | pred                                            # u_t on top of the predecessor's six bits
    sa, sb = 1 - 2 * _PARITY[window & _GEN_A], 1 - 2 * _PARITY[window & _GEN_B]   # [2, 64] of +-1
    metric = np.full((R, 64), -(1 << 30), dtype=np.int32)
    metric[:, 0] = 0
    decision = np.zeros((R, steps, 64), dtype=bool)
    for t in range(steps):
        za, zb = z[:, t, 0, None], z[:, t, 1, None]
        m0 = metric[:, pred[0]] + sa[0] * za + sb[0] * zb
        m1 = metric[:, pred[1]] + sa[1] * za + sb[1] * zb
        decision[:, t] = m1 > m0                                               # a tie takes r0
        metric = np.where(decision[:, t], m1, m0).astype(np.int32)
    state = np.zeros(R, dtype=np.int64)
    out = np.zeros((R, steps), dtype=np.uint8)
    rows = np.arange(R)
    for t in range(steps - 1, -1, -1):
        out[:, t] = state >> 5
        state = ((state & 31) << 1) | decision[rows, t, state]
    return out.reshape(*lead, steps)


def _decoder_input(code, keys: np.ndarray, llr: np.ndarray, sent: np.ndarray) -> np.ndarray:
    """int32 ``[n, B, coded_bits]``: the LLRs ``[n, S T, m]`` at the interleaver's positions, descrambled with the codewords ``sent``
    and quantised (a ``CodeConfig`` or an ``LdpcConfig``: the position on the link is the same)."""
    cfg = code.link
    m = cfg.bits_per_symbol
    j = code.positions()                                                       # [B, n]
    q, k = np.flatnonzero(cfg.data_mask)[j // m], j % m                        # the grid element and the bit of its word
    w = (words(keys[:, None, None], STREAM_DATA_BITS, q[None].astype(np.uint64)) >> (np.uint64(63) - k[None].astype(np.uint64))) & np.uint64(1)
    scrambler = w.astype(np.uint8) ^ sent
    at = llr[:, q, k]                                                          # [n, B, coded_bits]
    return quantise(np.where(scrambler == 1, -at, at), code.qgain)


def link_decode_host(code: CodeConfig, keys, llr) -> Tuple[np.ndarray, np.ndarray]:
    """The coded link's definition on ``llr`` ``[n, S, T, m]``, taken as the float32 numbers it rounds to: ``(counts int64 [n, 2] =
    (information-bit errors, blocks with any error) per frame, bits uint8 [n, B, K] the decoded information bits)``.  Needs no library."""
    keys = _keys64(keys)
    cfg = code.link
    (S, T), m, nf = cfg.sim.ofdm, cfg.bits_per_symbol, len(keys)
    llr = np.asarray(llr)
    if llr.shape != (nf, S, T, m):
        raise ValueError(f"Expected llr of shape ({nf}, {S}, {T}, {m}), got {llr.shape}")
    llr = llr.astype(np.float32).reshape(nf, S * T, m)
    info, sent = link_encode_host(code, keys)
    z = _decoder_input(code, keys, llr, sent)
    full = np.zeros((nf, code.blocks, code.steps, 2), dtype=np.int32)
    full[..., keep_mask(code.info_bits, code.rate)] = z
    bits = viterbi_host(full)[..., :code.info_bits]
    wrong = bits != info
    counts = np.stack([wrong.sum(axis=(1, 2)), wrong.any(axis=2).sum(axis=1)], axis=1).astype(np.int64)
    return counts, bits


class BlockErrorAccumulator(_FrameSweep):
    """Block errors of a sweep with a decoder in the loop (module docstring, "the coded link"), with ``LinkAccumulator``'s ``update``
    surface.  The LLRs are the soft link's at factor 1 with the scale ``llr_scale(snr_db, err_var)``.  On a HIP device a batch is the
    launch of ``aft_link_soft_f32`` with its LLR output, the launch of ``aft_link_decode_f32`` on that tensor, and one integer add into
    an int64 ``[2]`` device tensor; nothing synchronises.  On a CPU device the host definitions run (float64 LLRs rounded to float32).
    ``result`` is the block-error rate, ``result_ber`` the information-bit error rate, ``result_throughput`` the delivered information
    bits per data element; each is one read and, with several ranks, one all-gather of three float64.  ``branches``, ``streams``,
    ``detector`` and ``tx_diversity`` as ``LinkAccumulator``'s: with ``tx_diversity`` the LLRs are ``aft_link_alamouti_f32``'s (on a
    CPU device ``link_alamouti_host``'s) and the decoder reads them with the leaders' keys."""

    #: what ``LdpcBlockErrorAccumulator`` changes: the config it accepts, the host decoder, the decoder's plan and the columns of ``errors``
    _config, _needs, _host_decoder, _decoder_plan, _columns = CodeConfig, "a CodeConfig", staticmethod(link_decode_host), "LinkDecodePlan", 2

    def __init__(self, code, device, seed: int = 0, err_var: float = 0.0, branches: int = 1, streams: int = 1,
                 detector: str = "mmse", *, tx_diversity: Optional[str] = None, precoding_subband: Optional[int] = None,
                 precoding_delay: int = 0, slots: int = 1) -> None:
        if not isinstance(code, self._config):
            raise ValueError(f"{type(self).__name__} needs {self._needs} (got {type(code).__name__})")
        self._open(code.link, device, seed, "llr", branches, err_var, streams=streams, detector=detector, tx_diversity=tx_diversity,
                   precoding_subband=precoding_subband, precoding_delay=precoding_delay, slots=slots)
        self.code = code
        self.errors = torch.zeros(self._columns, dtype=torch.int64, device=self.device)    # information-bit errors, block errors, ...
        self._decode = None
        if self._plan is not None:
            from . import hip_ops
            self._decode = getattr(hip_ops, self._decoder_plan)(code, self.device)

    def _decoded(self, llr: torch.Tensor, keys: torch.Tensor) -> torch.Tensor:
        """The decoder's counts per group on the LLRs ``_measure`` returned: the host definition on a CPU device, the plan's launch on
        a HIP device."""
        if self._decode is None:
            return torch.from_numpy(self._host_decoder(self.code, keys.numpy(), llr.numpy())[0])
        return self._launch(llr, keys, plan=self._decode)[0]

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        got = self._measure(est, ideal, meta, frame_ids, snr_db)
        if got is not None:                        # the link's LLRs, then the decoder on the groups with the leaders' keys
            groups, keys, _, _, llr = got
            self.errors += self._total(self._decoded(llr, keys), torch.int64)
            self.frames += groups

    def _read(self, group) -> list:
        """The columns of ``errors``, then the frames, over all ranks."""
        frames = torch.tensor([float(self.frames)], dtype=torch.float64, device=self.device)
        return self._all_ranks(torch.cat([self.errors.to(torch.float64), frames]), group)

    def result(self, group: Optional["torch.distributed.ProcessGroup"] = None) -> float:
        """Global block-error rate over all ranks (integers summed: identical on every rank); 0.0 for an empty sweep."""
        _, block_errors, *_, frames = self._read(group)
        return block_errors / (frames * self.code.blocks) if frames > 0 else 0.0

    def result_ber(self, group=None) -> float:
        """Global information-bit error rate after decoding."""
        bit_errors, *_, frames = self._read(group)
        return bit_errors / (frames * self.code.info_bits_per_frame) if frames > 0 else 0.0

    def result_throughput(self, group=None) -> float:
        """Information bits of the blocks decoded without error, per data element sent."""
        _, block_errors, *_, frames = self._read(group)
        if frames <= 0:
            return 0.0
        return (frames * self.code.blocks - block_errors) * self.code.info_bits / (frames * self.cfg.data_elements)


# ---- the LDPC-coded link (module docstring, "the LDPC-coded link"): integer NumPy, mirrored by csrc/k_linkldpc.hip ----

LDPC_Z = _abi.AFT_LINK_LDPC_Z
LDPC_MAX_EDGES = _abi.AFT_LINK_LDPC_MAX_EDGES
LDPC_MIN_ROWS, LDPC_MAX_ROWS, LDPC_MAX_COLS = 3, 16, 32
LDPC_RATES = {"1/2": (12, 24), "2/3": (8, 24), "3/4": (6, 24)}
LDPC_L_MAX, LDPC_R_MAX = 8191, 127                           # posteriors fit int16, messages int8


def _ldpc_shape(mb, nb) -> Tuple[int, int]:
    for name, v in (("mb", mb), ("nb", nb)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{name} = {v!r}: an integer")
    mb, nb = int(mb), int(nb)
    if not LDPC_MIN_ROWS <= mb <= LDPC_MAX_ROWS:
        raise ValueError(f"mb = {mb}: a base matrix has {LDPC_MIN_ROWS} .. {LDPC_MAX_ROWS} rows")
    if not mb < nb <= LDPC_MAX_COLS:
        raise ValueError(f"nb = {nb}: a base matrix of {mb} rows has {mb + 1} .. {LDPC_MAX_COLS} columns")
    return mb, nb


def ldpc_parity_part(mb: int) -> np.ndarray:
    """int32 ``[mb, mb]``: the parity columns ``kb .. nb-1`` of every base matrix of ``mb`` rows (-1: no block)."""
    P = np.full((mb, mb), -1, dtype=np.int32)
    P[0, 0] = P[mb - 1, 0] = 1
    P[mb // 2, 0] = 0
    for i in range(mb - 1):
        P[i, 1 + i] = P[i + 1, 1 + i] = 0
    return P


def ldpc_base(mb: int, nb: int, seed: int = 0) -> np.ndarray:
    """int32 ``[mb, nb - mb]``: the default information part (module docstring): three entries per column, their shifts from stream 9
    of the hash of ``seed``, moved on to the first value that closes no 4-cycle."""
    mb, nb = _ldpc_shape(mb, nb)
    kb = nb - mb
    S = np.full((mb, nb), -1, dtype=np.int64)
    S[:, kb:] = ldpc_parity_part(mb)
    offsets = (0, 1, mb // 2 - 1) if mb >= 8 else (0, 1, 2)
    key = np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    for j in range(kb):
        for t in range(3):
            r = (j + offsets[t]) % mb
            h = int(words(key, STREAM_LDPC_SHIFTS, 4 * j + t)[0] >> np.uint64(58))
            refused = set()
            for r2 in range(mb):
                if r2 == r or S[r2, j] < 0:
                    continue
                for b in range(nb):
                    if b != j and S[r, b] >= 0 and S[r2, b] >= 0:
                        refused.add(int(S[r2, j] + S[r, b] - S[r2, b]) % LDPC_Z)
            for c in range(LDPC_Z):
                if (h + c) % LDPC_Z not in refused:
                    S[r, j] = (h + c) % LDPC_Z
                    break
            else:
                raise ValueError(f"ldpc_base({mb}, {nb}, seed={seed}): no shift without a 4-cycle at row {r} of column {j}")
    return S[:, :kb].astype(np.int32)


@dataclass(frozen=True)
class LdpcConfig:
    """A quasi-cyclic LDPC code (lifting 64) on a link: ``rate`` one of ``LDPC_RATES`` or ``(mb, nb)``, ``shifts`` the information part
    int ``[mb][nb - mb]`` (None: ``ldpc_base(mb, nb, seed)``), the interleaver's ``stride`` (None: the golden-section default), the
    quantiser's gain, the min-sum ``offset`` and ``max_iters``.  Derives what ``CodeConfig`` derives, plus ``base()`` and ``edges``;
    refuses what ``aft_link_ldpc_f32`` refuses."""
    link: LinkConfig = field(default_factory=LinkConfig)
    rate: Union[str, Tuple[int, int]] = "1/2"
    shifts: Optional[tuple] = None
    seed: int = 0
    stride: Optional[int] = None
    qgain: float = 8.0
    offset: int = 4
    max_iters: int = 20

    def __post_init__(self) -> None:
        if not isinstance(self.link, LinkConfig):
            raise ValueError(f"LdpcConfig needs a LinkConfig (got {type(self.link).__name__})")
        if isinstance(self.rate, str):
            if self.rate not in LDPC_RATES:
                raise ValueError(f"rate = {self.rate!r}: one of {tuple(LDPC_RATES)}, or (mb, nb)")
            mb, nb = LDPC_RATES[self.rate]
        else:
            try:
                mb, nb = self.rate
            except (TypeError, ValueError):
                raise ValueError(f"rate = {self.rate!r}: one of {tuple(LDPC_RATES)}, or (mb, nb)") from None
            mb, nb = _ldpc_shape(mb, nb)
            object.__setattr__(self, "rate", (mb, nb))
        object.__setattr__(self, "_shape", (mb, nb))
        kb = nb - mb
        if self.shifts is None:
            table = ldpc_base(mb, nb, self.seed)
        else:
            table = np.asarray(self.shifts)
            if table.shape != (mb, kb) or table.dtype.kind not in "iu":
                raise ValueError(f"shifts: an integer table [{mb}][{kb}], got {table.dtype} {table.shape}")
            if table.size and (table.min() < -1 or table.max() >= LDPC_Z):
                raise ValueError(f"shifts: every entry is -1 (no block) or a shift in 0 .. {LDPC_Z - 1}")
            empty = np.flatnonzero((table >= 0).sum(axis=0) == 0)
            if empty.size:
                raise ValueError(f"shifts: base column {int(empty[0])} has no entry")
        object.__setattr__(self, "shifts", tuple(tuple(int(v) for v in row) for row in table))
        if self.edges > LDPC_MAX_EDGES:
            raise ValueError(f"shifts: {self.edges} entries in the base matrix, parity part included; at most {LDPC_MAX_EDGES}")
        if self.blocks == 0:
            raise ValueError(f"a frame carries {self.link.bits_per_frame} bits, fewer than the {self.coded_bits} coded bits of one block")
        if self.info_bits_per_frame > 1 << 31:
            raise ValueError(f"{self.blocks} blocks of {self.info_bits} information bits: more than 2^31, where the hash's index and the "
                             f"int32 counts end")
        U = self.used_bits
        a = default_stride(U) if self.stride is None else self.stride
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 1 <= int(a) < U:
            raise ValueError(f"stride = {a!r}: an integer in [1, {U})")
        if math.gcd(int(a), U) != 1:
            raise ValueError(f"stride = {a} is not coprime to the {U} used bits")
        object.__setattr__(self, "stride", int(a))
        with np.errstate(over="ignore", under="ignore"):
            g = np.float32(self.qgain)
        if not (np.isfinite(g) and g > 0):
            raise ValueError(f"qgain = {self.qgain!r}: a finite positive float32")
        object.__setattr__(self, "qgain", float(g))
        for name, lo, hi in (("offset", 0, LDPC_R_MAX), ("max_iters", 1, 255)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} = {v!r}: an integer in {lo} .. {hi}")
            object.__setattr__(self, name, int(v))

    @property
    def base_rows(self) -> int:
        return self._shape[0]

    @property
    def base_cols(self) -> int:
        return self._shape[1]

    @property
    def info_bits(self) -> int:
        return LDPC_Z * (self.base_cols - self.base_rows)

    @property
    def coded_bits(self) -> int:
        return LDPC_Z * self.base_cols

    @property
    def blocks(self) -> int:
        return self.link.bits_per_frame // self.coded_bits

    @property
    def used_bits(self) -> int:
        return self.blocks * self.coded_bits

    @property
    def stride_inverse(self) -> int:
        return pow(self.stride, -1, self.used_bits)

    @property
    def info_bits_per_frame(self) -> int:
        return self.blocks * self.info_bits

    @property
    def edges(self) -> int:
        """The entries of the whole base matrix, parity part included."""
        return int((self.base() >= 0).sum())

    positions = CodeConfig.positions

    def base(self) -> np.ndarray:
        """int32 ``[mb, nb]``: the information part beside the parity part."""
        mb, nb = self._shape
        return np.concatenate([np.asarray(self.shifts, dtype=np.int32).reshape(mb, nb - mb), ldpc_parity_part(mb)], axis=1)

    def layers(self):
        """Per layer ``(cols int64 [d], var int64 [d, 64])``: its edges in increasing column order and, for each of its 64 rows
        ``r``, the variable ``64 j + ((r + s) mod 64)`` of every edge."""
        out, r = [], np.arange(LDPC_Z)
        for row in self.base():
            cols = np.flatnonzero(row >= 0)
            out.append((cols, LDPC_Z * cols[:, None] + (r[None, :] + row[cols][:, None]) % LDPC_Z))
        return out


def ldpc_encode(cfg: LdpcConfig, u) -> np.ndarray:
    """The codewords uint8 ``[..., n]`` of the information bits ``u`` ``[..., K]`` (0 / 1): ``u | p_0 | .. | p_{mb-1}``."""
    u = np.asarray(u).astype(np.uint8)
    mb, nb = cfg.base_rows, cfg.base_cols
    kb, mid = nb - mb, mb // 2
    if u.shape[-1] != cfg.info_bits:
        raise ValueError(f"Expected {cfg.info_bits} information bits on the last axis, got {u.shape}")
    blocks = u.reshape(*u.shape[:-1], kb, LDPC_Z)
    rot = lambda x, s: np.roll(x, -int(s), axis=-1)  # noqa: E731  rot(x, s)[r] = x[(r + s) mod 64]
    lam = np.zeros((*u.shape[:-1], mb, LDPC_Z), dtype=np.uint8)
    for i, row in enumerate(cfg.shifts):
        for j, s in enumerate(row):
            if s >= 0:
                lam[..., i, :] ^= rot(blocks[..., j, :], s)
    p = np.zeros_like(lam)
    p[..., 0, :] = np.bitwise_xor.reduce(lam, axis=-2)
    p[..., 1, :] = lam[..., 0, :] ^ rot(p[..., 0, :], 1)
    for i in range(1, mb - 1):
        p[..., i + 1, :] = lam[..., i, :] ^ p[..., i, :] ^ (p[..., 0, :] if i == mid else 0)
    return np.concatenate([u, p.reshape(*u.shape[:-1], mb * LDPC_Z)], axis=-1)


def link_ldpc_encode_host(cfg: LdpcConfig, keys) -> Tuple[np.ndarray, np.ndarray]:
    """The information bits uint8 ``[n, B, K]`` and the codewords uint8 ``[n, B, coded_bits]`` of the frames with ``keys``."""
    keys = _keys64(keys)
    B, K = cfg.blocks, cfg.info_bits
    index = np.arange(B * K, dtype=np.uint64).reshape(1, B, K)
    info = (words(keys[:, None, None], STREAM_CODE_BITS, index) >> np.uint64(63)).astype(np.uint8)
    return info, ldpc_encode(cfg, info)


def ldpc_syndrome_ok(cfg: LdpcConfig, x: np.ndarray) -> np.ndarray:
    """bool ``[...]``: whether the hard bits ``x`` ``[..., n]`` satisfy all ``64 mb`` checks."""
    x = np.asarray(x).astype(bool)
    ok = np.ones(x.shape[:-1], dtype=bool)
    for _, var in cfg.layers():
        ok &= ~np.logical_xor.reduce(x[..., var], axis=-2).any(axis=-1)
    return ok


def ldpc_decode_host(cfg: LdpcConfig, z) -> Tuple[np.ndarray, np.ndarray]:
    """The decoder of the definition on quantised inputs ``z`` int ``[..., n]``: ``(bits uint8 [..., K], iterations int64 [...])``.
    Vectorised over the blocks and over the 64 rows of a layer; a block that has stopped is left alone."""
    z = np.asarray(z, dtype=np.int32)
    if z.shape[-1] != cfg.coded_bits:
        raise ValueError(f"Expected {cfg.coded_bits} inputs on the last axis, got {z.shape}")
    lead = z.shape[:-1]
    L = z.reshape(-1, cfg.coded_bits).copy()
    layers = cfg.layers()
    msg = [np.zeros((L.shape[0], *var.shape), dtype=np.int32) for _, var in layers]
    iterations = np.zeros(L.shape[0], dtype=np.int64)
    active = np.arange(L.shape[0])
    beta = cfg.offset
    for it in range(1, cfg.max_iters + 1):
        if active.size == 0:
            break
        La = L[active]
        for i, (cols, var) in enumerate(layers):
            Q = La[:, var] - msg[i][active]                                    # [A, d, 64]: all Q of the layer before any update
            neg, mag = Q < 0, np.abs(Q)
            tot = np.logical_xor.reduce(neg, axis=1, keepdims=True)
            a = mag.argmin(axis=1)[:, None, :]                                 # the lowest e that attains the minimum
            m1 = np.take_along_axis(mag, a, axis=1)
            rest = mag.copy()
            np.put_along_axis(rest, a, np.iinfo(np.int32).max, axis=1)
            m2 = rest.min(axis=1, keepdims=True)
            is_a = np.arange(len(cols))[None, :, None] == a
            out = np.clip(np.where(is_a, m2, m1) - beta, 0, LDPC_R_MAX)
            R = np.where(tot ^ neg, -out, out).astype(np.int32)
            La[:, var] = np.clip(Q + R, -LDPC_L_MAX, LDPC_L_MAX)
            msg[i][active] = R
        L[active] = La
        iterations[active] = it
        active = active[~ldpc_syndrome_ok(cfg, La < 0)]
    bits = (L[:, :cfg.info_bits] < 0).astype(np.uint8)
    return bits.reshape(*lead, cfg.info_bits), iterations.reshape(lead)


def link_ldpc_host(cfg: LdpcConfig, keys, llr) -> Tuple[np.ndarray, np.ndarray]:
    """The LDPC-coded link's definition on ``llr`` ``[n, S, T, m]``, taken as the float32 numbers it rounds to: ``(counts int64 [n, 3] =
    (information-bit errors, blocks with any error, iterations summed over the blocks) per frame, bits uint8 [n, B, K])``.  Needs no
    library."""
    if not isinstance(cfg, LdpcConfig):
        raise ValueError(f"link_ldpc_host needs an LdpcConfig (got {type(cfg).__name__})")
    keys = _keys64(keys)
    (S, T), m, nf = cfg.link.sim.ofdm, cfg.link.bits_per_symbol, len(keys)
    llr = np.asarray(llr)
    if llr.shape != (nf, S, T, m):
        raise ValueError(f"Expected llr of shape ({nf}, {S}, {T}, {m}), got {llr.shape}")
    llr = llr.astype(np.float32).reshape(nf, S * T, m)
    info, sent = link_ldpc_encode_host(cfg, keys)
    bits, iterations = ldpc_decode_host(cfg, _decoder_input(cfg, keys, llr, sent))
    wrong = bits != info
    counts = np.stack([wrong.sum(axis=(1, 2)), wrong.any(axis=2).sum(axis=1), iterations.sum(axis=1)], axis=1).astype(np.int64)
    return counts, bits


class LdpcBlockErrorAccumulator(BlockErrorAccumulator):
    """``BlockErrorAccumulator`` for an ``LdpcConfig``: the same ``update`` surface and results, an int64 ``[3]`` device tensor
    (information-bit errors, block errors, iterations) and ``result_iterations``, the mean iterations per block.  On a HIP device a
    batch is the launch of ``aft_link_soft_f32`` with its LLR output, the launch of ``aft_link_ldpc_f32`` on that tensor and one
    integer add; nothing synchronises.  On a CPU device the host definitions run.  Each result is one read and, with several ranks,
    one all-gather of four float64.  ``branches``, ``streams``, ``detector`` and ``tx_diversity`` as ``BlockErrorAccumulator``'s; with
    ``streams=2`` this accumulator alone also takes ``detector="cwsic"``, codeword-level cancellation (``__init__``)."""

    _config, _needs, _host_decoder, _decoder_plan, _columns = LdpcConfig, "an LdpcConfig", staticmethod(link_ldpc_host), "LinkLdpcPlan", 3
    _runs_cwsic = True

    def __init__(self, code, device, seed: int = 0, err_var: float = 0.0, branches: int = 1, streams: int = 1,
                 detector: str = "mmse", *, tx_diversity: Optional[str] = None, precoding_subband: Optional[int] = None,
                 precoding_delay: int = 0, slots: int = 1) -> None:
        """``streams=2, detector="cwsic"`` (module docstring, "the codeword-cancellation link"): MMSE detection and decoding of both
        streams, then a stream that failed while the other passed is detected again with the acknowledged codeword cancelled, and decoded
        again.  On a HIP device a batch is four launches -- ``aft_link_sm_f32``, ``aft_link_ldpc_f32``, ``aft_link_cancel_f32`` reading
        the decoder's block errors in place, ``aft_link_ldpc_masked_f32`` reading the cancel kernel's flags -- and a ``torch.where`` and
        three integer adds on the device; nothing synchronises.  On a CPU device ``link_cwsic_host`` runs.  ``result``, ``result_ber``
        and ``result_throughput`` give the values AFTER cancellation, ``result_iterations`` both passes summed, ``result_first_pass`` the
        block-error rate before cancellation (the ``detector="mmse"`` sweep's ``result``) and ``cwsic_stats`` what the second pass did."""
        super().__init__(code, device, seed, err_var, branches, streams, detector, tx_diversity=tx_diversity,
                         precoding_subband=precoding_subband, precoding_delay=precoding_delay, slots=slots)
        if self._cwsic:
            self._first = torch.zeros(3, dtype=torch.int64, device=self.device)          # the first pass's three counts
            self._second = torch.zeros(3, dtype=torch.int64, device=self.device)         # streams detected again; of those decoded; groups both failed
            self._cancel = None
            if self._plan is not None:
                from . import hip_ops
                self._cancel = hip_ops.LinkCancelPlan(code.link, self.device, self.branches, self.streams)

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        if not self._cwsic:
            return super().update(est, ideal, meta, frame_ids=frame_ids, snr_db=snr_db)
        ops = self._operands(est, ideal, meta, frame_ids, snr_db, self._of_snr)
        if ops is None:
            return
        b, H, E, keys, (sigma, scale) = ops
        R, N = self.branches, self.streams
        G = _grouped(b, R, N)
        if self._plan is None:                     # the host twins, whole
            rho, lead = _weights(scale, R * N)
            first, redo, second, _ = link_cwsic_host(self.code, keys, H, E, sigma, rho, lead, detector_reg(lead, "mmse"), R)
            first, second = (torch.from_numpy(v.reshape(G * N, 3)) for v in (first, second))
            redo = torch.from_numpy(redo.reshape(G * N))
        else:                                      # four launches; every operand of a later one is an earlier one's output, in place
            rho, lead = self._device_weights(scale, R * N)
            reg = (1.0 / lead.to(torch.float64)).to(torch.float32)
            sent = keys.view(G, R, N)[:, 0, :].reshape(-1)
            llr = self._launch(H, E, keys, sigma, rho, lead, reg, self._factors_t, want_llr=True)[2]
            first = self._launch(llr, sent, plan=self._decode)[0]
            _, _, llr, state = self._launch(H, E, keys, sigma, rho, lead, first[:, 1], self._factors_t, want_llr=True, plan=self._cancel)
            second = self._launch(llr, sent, plan=self._decode, mask=state.view(-1))[0]
            redo = state.view(-1) != 0
        final = torch.where(redo[:, None], second, first)
        final[:, 2] = first[:, 2] + second[:, 2]                                         # a stream without redo ran no second pass: 0
        both = (first[:, 1].reshape(G, N) != 0).all(dim=1)
        self.errors += self._total(final, torch.int64)
        self._first += self._total(first, torch.int64)
        self._second += torch.stack([redo.sum(), (redo & (second[:, 1] == 0)).sum(), both.sum()]).to(torch.int64)
        self.frames += G * N

    def _need_cwsic(self, what: str) -> None:
        if not self._cwsic:
            raise ValueError(f'{what} needs streams=2 and detector="cwsic": no other link decodes twice')

    def result_first_pass(self, group=None) -> float:
        """The block-error rate BEFORE cancellation over all ranks: what ``detector="mmse"`` gives on the same updates."""
        self._need_cwsic("result_first_pass")
        frames = torch.tensor([float(self.frames)], dtype=torch.float64, device=self.device)
        _, block_errors, _, frames = self._all_ranks(torch.cat([self._first.to(torch.float64), frames]), group)
        return block_errors / (frames * self.code.blocks) if frames > 0 else 0.0

    def cwsic_stats(self, group=None) -> tuple:
        """What the second pass did over the sweep, all ranks: ``(the share of streams detected again, the share of those streams then
        decoded without a block error, the share of groups in which both streams failed -- where nothing can be cancelled)``; 0.0 where
        a denominator is 0.  Summed on the device by one add per batch; one read, as the result's."""
        self._need_cwsic("cwsic_stats")
        frames = torch.tensor([float(self.frames)], dtype=torch.float64, device=self.device)
        again, decoded, both, frames = self._all_ranks(torch.cat([self._second.to(torch.float64), frames]), group)
        groups = frames / self.streams
        return (again / frames if frames > 0 else 0.0, decoded / again if again > 0 else 0.0, both / groups if groups > 0 else 0.0)

    def result_iterations(self, group=None) -> float:
        """Mean decoder iterations per block over all ranks -- with ``detector="cwsic"`` both passes summed --; 0.0 for an empty sweep."""
        _, _, iterations, frames = self._read(group)
        return iterations / (frames * self.code.blocks) if frames > 0 else 0.0


# ---- the HARQ link (module docstring, "The HARQ link"): integer NumPy, mirrored by csrc/k_linkharq.hip ----

HARQ_MAX_ROUNDS = _abi.AFT_LINK_HARQ_MAX_ROUNDS
HARQ_COUNTS = _abi.AFT_LINK_HARQ_COUNTS
HARQ_MODES = ("ir", "chase")


@dataclass(frozen=True)
class HarqConfig:
    """Hybrid ARQ on an LDPC-coded link: the mother code ``code`` (an ``LdpcConfig``, valid on its link), ``tx_cols`` = C of its nb block
    columns per round, ``rounds`` = Q, the windows' ``starts`` (None: those of ``mode``, "ir" continuing round by round or "chase"
    repeating the first) and the interleaver's ``stride`` over the ``B E`` used bits (None: the golden-section default).  Derives
    ``tx_bits`` E, ``blocks`` B, ``used_bits`` U, ``stride_inverse``, ``info_bits_per_frame``, ``windows()`` and ``positions()``;
    refuses what ``aft_link_harq_f32`` refuses."""
    code: LdpcConfig
    tx_cols: int
    rounds: int = HARQ_MAX_ROUNDS
    starts: Optional[tuple] = None
    mode: str = "ir"
    stride: Optional[int] = None

    def __post_init__(self) -> None:
        if not isinstance(self.code, LdpcConfig):
            raise ValueError(f"HarqConfig needs an LdpcConfig as its mother code (got {type(self.code).__name__})")
        mb, nb = self.code.base_rows, self.code.base_cols
        kb = nb - mb
        for name, lo, hi in (("tx_cols", kb + 1, nb), ("rounds", 1, HARQ_MAX_ROUNDS)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
                raise ValueError(f"{name} = {v!r}: an integer in {lo} .. {hi}")
            object.__setattr__(self, name, int(v))
        if self.mode not in HARQ_MODES:
            raise ValueError(f"mode = {self.mode!r}: one of {HARQ_MODES}")
        if self.starts is None:
            starts = [(t * self.tx_cols) % nb if self.mode == "ir" else 0 for t in range(self.rounds)]
        else:
            try:
                starts = list(self.starts)
            except TypeError:
                raise ValueError(f"starts = {self.starts!r}: {self.rounds} block columns, one per round") from None
            if len(starts) != self.rounds:
                raise ValueError(f"starts = {self.starts!r}: {self.rounds} block columns, one per round")
            for s in starts:
                if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < nb:
                    raise ValueError(f"starts = {self.starts!r}: every start is a block column in 0 .. {nb - 1}")
        object.__setattr__(self, "starts", tuple(int(s) for s in starts))
        if self.blocks == 0:
            raise ValueError(f"a frame carries {self.link.bits_per_frame} bits, fewer than the {self.tx_bits} coded bits of one block")
        if self.info_bits_per_frame > 1 << 31:
            raise ValueError(f"{self.blocks} blocks of {self.info_bits} information bits: more than 2^31, where the hash's index and the "
                             f"int32 counts end")
        U = self.used_bits
        a = default_stride(U) if self.stride is None else self.stride
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not 1 <= int(a) < U:
            raise ValueError(f"stride = {a!r}: an integer in [1, {U})")
        if math.gcd(int(a), U) != 1:
            raise ValueError(f"stride = {a} is not coprime to the {U} used bits")
        object.__setattr__(self, "stride", int(a))

    @property
    def link(self) -> LinkConfig:
        return self.code.link

    @property
    def info_bits(self) -> int:
        return self.code.info_bits

    @property
    def tx_bits(self) -> int:
        """E: the coded bits of a block one round sends."""
        return LDPC_Z * self.tx_cols

    @property
    def blocks(self) -> int:
        return self.link.bits_per_frame // self.tx_bits

    @property
    def used_bits(self) -> int:
        return self.blocks * self.tx_bits

    @property
    def stride_inverse(self) -> int:
        return pow(self.stride, -1, self.used_bits)

    @property
    def info_bits_per_frame(self) -> int:
        return self.blocks * self.info_bits

    def windows(self) -> np.ndarray:
        """int64 ``[Q, E]``: the codeword bit ``v_t(e)`` behind transmitted bit ``e`` of round ``t``."""
        e = np.arange(self.tx_bits, dtype=np.int64)
        s = np.asarray(self.starts, dtype=np.int64)[:, None]
        return LDPC_Z * ((s + e[None, :] // LDPC_Z) % self.code.base_cols) + e[None, :] % LDPC_Z

    def positions(self) -> np.ndarray:
        """int64 ``[B, E]``: the data-bit index ``j = ((b E + e) stride) mod U`` of transmitted bit ``e`` of block ``b``."""
        U, p = self.used_bits, np.arange(self.used_bits, dtype=np.int64)
        if U <= 1 << 31:
            j = (p * np.int64(self.stride)) % np.int64(U)
        else:
            j = np.array([(int(v) * self.stride) % U for v in p], dtype=np.int64)
        return j.reshape(self.blocks, self.tx_bits)


def link_harq_host(harq: HarqConfig, keys, llr) -> Tuple[np.ndarray, np.ndarray]:
    """The HARQ link's definition on ``llr`` ``[G Q, S, T, m]``, taken as the float32 numbers it rounds to, with the ``G Q`` ``keys``:
    ``(counts int64 [G, 7], bits uint8 [G, B, K])`` (module docstring, "The HARQ link").  Needs no library."""
    if not isinstance(harq, HarqConfig):
        raise ValueError(f"link_harq_host needs a HarqConfig (got {type(harq).__name__})")
    keys = _keys64(keys)
    code, cfg, Q = harq.code, harq.link, harq.rounds
    (S, T), m, nf = cfg.sim.ofdm, cfg.bits_per_symbol, len(keys)
    if nf == 0 or nf % Q:
        raise ValueError(f"a batch of {nf} frames is not a positive multiple of rounds = {Q}")
    llr = np.asarray(llr)
    if llr.shape != (nf, S, T, m):
        raise ValueError(f"Expected llr of shape ({nf}, {S}, {T}, {m}), got {llr.shape}")
    llr = llr.astype(np.float32).reshape(nf, S * T, m)
    G, B, K = nf // Q, harq.blocks, harq.info_bits
    index = np.arange(B * K, dtype=np.uint64).reshape(1, B, K)
    info = (words(keys[::Q, None, None], STREAM_CODE_BITS, index) >> np.uint64(63)).astype(np.uint8)     # the leaders'
    sent = ldpc_encode(code, info)                                                # [G, B, n]
    j = harq.positions()                                                          # [B, E]
    q, k = np.flatnonzero(cfg.data_mask)[j // m], j % m
    Z = np.zeros((G, B, code.coded_bits), dtype=np.int32)
    acked = np.zeros((G, B), dtype=bool)
    bits = np.zeros((G, B, K), dtype=np.uint8)
    counts = np.zeros((G, HARQ_COUNTS), dtype=np.int64)
    for t, v in enumerate(harq.windows()):                                        # a round's window holds every variable at most once
        kt = keys[t::Q]
        w = (words(kt[:, None, None], STREAM_DATA_BITS, q[None].astype(np.uint64)) >> (np.uint64(63) - k[None].astype(np.uint64))) & np.uint64(1)
        scrambler = w.astype(np.uint8) ^ sent[:, :, v]
        at = llr[t::Q][:, q, k]                                                   # [G, B, E]
        Z[:, :, v] += quantise(np.where(scrambler == 1, -at, at), code.qgain)
        todo = ~acked
        if not todo.any():
            break
        got, iterations = ldpc_decode_host(code, Z[todo])
        bits[todo] = got
        ok = (got == info[todo]).all(axis=-1)
        ran = np.zeros((G, B), dtype=np.int64)
        ran[todo] = iterations
        counts[:, 6] += ran.sum(axis=1)
        first = np.zeros((G, B), dtype=bool)
        first[todo] = ok
        counts[:, t] = first.sum(axis=1)
        acked |= first
    wrong = (bits != info) & ~acked[:, :, None]
    counts[:, 4] = wrong.sum(axis=(1, 2))
    counts[:, 5] = (~acked).sum(axis=1)
    return counts, bits


class HarqAccumulator(BlockErrorAccumulator):
    """A sweep under hybrid ARQ (module docstring, "The HARQ link") with ``BlockErrorAccumulator``'s ``update`` surface: a batch holds a
    multiple of ``branches * rounds`` frames; the link's LLRs -- the combiner's, with branches -- and the leaders' keys are grouped
    ``rounds`` at a time.  On a HIP device a batch is the launch that writes the LLRs, the launch of ``aft_link_harq_f32`` on that
    tensor and one integer add into an int64 ``[7]`` device tensor; nothing synchronises.  On a CPU device the host definitions run.
    ``result`` is the residual block-error rate after all rounds, ``result_bler_after(t)`` the one after round t,
    ``result_transmissions`` the mean rounds a block used (a failed block counts all Q), ``result_throughput`` the delivered
    information bits per data element actually sent and ``result_iterations`` the mean iterations per block over all its attempts;
    each is one read and, with several ranks, one all-gather of eight float64."""

    _config, _needs, _host_decoder, _decoder_plan, _columns = HarqConfig, "a HarqConfig", staticmethod(link_harq_host), "LinkHarqPlan", HARQ_COUNTS

    def __init__(self, code, device, seed: int = 0, err_var: float = 0.0, branches: int = 1, **unknown) -> None:
        # no ``streams``: a group's rounds are consecutive LLR frames, which would be the two streams of one group; no ``tx_diversity``
        # and no ``precoding_subband``: HARQ over Alamouti pairs or precoded transmissions is not defined here; no ``detector``: one
        # stream has none.  A keyword it does not have stays a TypeError; ``detector="cwsic"`` is told where codeword cancellation runs
        if unknown:
            _refuse_cwsic(unknown.get("detector"), "HarqAccumulator", "HARQ runs on one stream, combined over `branches`")
            raise TypeError(f"HarqAccumulator.__init__() got an unexpected keyword argument {next(iter(unknown))!r}")
        super().__init__(code, device, seed, err_var, branches)

    def update(self, est: Optional[torch.Tensor], ideal: torch.Tensor, meta: Optional[tuple] = None, *, frame_ids=None,
               snr_db=None) -> None:
        if ideal.dim() >= 1 and ideal.shape[0] % (self.branches * self.code.rounds):
            raise ValueError(f"a batch of {ideal.shape[0]} frames is not a multiple of branches * rounds = "
                             f"{self.branches} * {self.code.rounds}")
        super().update(est, ideal, meta, frame_ids=frame_ids, snr_db=snr_db)

    def _tally(self, group):
        """``(acked per round [4], blocks never acknowledged, iterations, all blocks)`` over all ranks: the blocks are counted, not
        derived from the frames."""
        *acked, _, failed, iterations, _ = self._read(group)
        return acked, failed, iterations, sum(acked) + failed

    def result(self, group: Optional["torch.distributed.ProcessGroup"] = None) -> float:
        """Global residual block-error rate after all rounds (integers summed: identical on every rank); 0.0 for an empty sweep."""
        _, failed, _, blocks = self._tally(group)
        return failed / blocks if blocks > 0 else 0.0

    def result_bler_after(self, t: int, group=None) -> float:
        """The share of blocks not yet acknowledged after round ``t`` in 0 .. Q-1."""
        if isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) < self.code.rounds:
            raise ValueError(f"t = {t!r}: a round in 0 .. {self.code.rounds - 1}")
        acked, _, _, blocks = self._tally(group)
        return (blocks - sum(acked[:int(t) + 1])) / blocks if blocks > 0 else 0.0

    def result_ber(self, group=None) -> float:
        """Global residual information-bit error rate: the errors of the blocks never acknowledged over all information bits."""
        bit_errors = self._read(group)[4]
        _, _, _, blocks = self._tally(group)
        return bit_errors / (blocks * self.code.info_bits) if blocks > 0 else 0.0

    def _rounds_used(self, group):
        acked, failed, _, blocks = self._tally(group)
        return sum((t + 1) * a for t, a in enumerate(acked)) + self.code.rounds * failed, sum(acked), blocks

    def result_transmissions(self, group=None) -> float:
        """Mean rounds used per block; a block never acknowledged counts all Q."""
        used, _, blocks = self._rounds_used(group)
        return used / blocks if blocks > 0 else 0.0

    def result_throughput(self, group=None) -> float:
        """Information bits of the acknowledged blocks per data element actually sent: a block's round takes 1 / B of a frame."""
        used, acked, blocks = self._rounds_used(group)
        return self.code.info_bits * acked * self.code.blocks / (self.cfg.data_elements * used) if blocks > 0 else 0.0

    def result_iterations(self, group=None) -> float:
        """Mean decoder iterations per block, summed over all its attempts."""
        _, _, iterations, blocks = self._tally(group)
        return iterations / blocks if blocks > 0 else 0.0
