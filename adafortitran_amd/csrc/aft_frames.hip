// aft_frames.hip -- the C ABI of the one-workgroup-per-frame kernels: the channel simulator, the LMMSE baseline and the link-level error
// counts (single-branch, with receive diversity, coded).  Their structs start with the same four fields and two carry the pilot
// positions, so those checks are written once.
#include <initializer_list>

#include "aft_internal.h"

using namespace aft;

namespace {

bool within(const char *who, const char *what, int got, int least, int most) {
    if (got < least || got > most) set_error("%s: %s = %d is outside %d..%d", who, what, got, least, most);
    return got >= least && got <= most;
}

// num_scs, num_symbols in 1 .. most (the caller's bound), the pilot grid inside the bounds the kernels' LDS is sized for
template <class Frame>
bool grid_ok(const char *who, const Frame &f, int most) {
    return within(who, "num_scs", f.num_scs, 1, most) && within(who, "num_symbols", f.num_symbols, 1, most) &&
           within(who, "pilot_scs", f.pilot_scs, 1, AFT_CHANSIM_MAX_PILOT_SCS) &&
           within(who, "pilot_symbols", f.pilot_symbols, 1, AFT_CHANSIM_MAX_PILOT_SYMBOLS);
}

template <class Frame>
bool pilots_fit(const char *who, const Frame &f) {
    if (f.pilot_scs <= f.num_scs && f.pilot_symbols <= f.num_symbols) return true;
    set_error("%s: the pilot grid %d x %d is larger than the ofdm grid %d x %d", who, f.pilot_scs, f.pilot_symbols, f.num_scs, f.num_symbols);
    return false;
}

// index[0 .. n) inside [0, size), `unit` of them; increasing: and each above the one before it
bool index_ok(const char *who, const char *what, const int32_t *index, int n, int size, const char *unit, bool increasing) {
    for (int i = 0; i < n; ++i) {
        if (index[i] >= 0 && index[i] < size && !(increasing && i > 0 && index[i] <= index[i - 1])) continue;
        if (increasing) set_error("%s: %s[%d] = %d: the positions must be strictly increasing inside [0, %d)", who, what, i, index[i], size);
        else set_error("%s: %s[%d] = %d is outside the grid's %d %s", who, what, i, index[i], size, unit);
        return false;
    }
    return true;
}

template <class Frame>
bool pilot_index_ok(const char *who, const Frame &f, bool increasing) {
    return index_ok(who, "pilot_sc_index", f.pilot_sc_index, f.pilot_scs, f.num_scs, "subcarriers", increasing) &&
           index_ok(who, "pilot_symbol_index", f.pilot_symbol_index, f.pilot_symbols, f.num_symbols, "symbols", increasing);
}

// the plan's own checks, shared by the size query and the launch; 0 = fine
int check_lmmse(const aft_lmmse *p) {
    const char *who = "lmmse";
    if (!grid_ok(who, *p, 1 << 20) || !within(who, "n_snr", p->n_snr, 1, AFT_CHANSIM_MAX_VALUES) ||
        !within(who, "n_ds", p->n_ds, 1, AFT_CHANSIM_MAX_VALUES) || !within(who, "n_dop", p->n_dop, 1, AFT_CHANSIM_MAX_VALUES) ||
        !within(who, "fixed_snr", p->fixed_snr, -1, p->n_snr - 1) || !within(who, "fixed_ds", p->fixed_ds, -1, p->n_ds - 1) ||
        !within(who, "fixed_dop", p->fixed_dop, -1, p->n_dop - 1) || !pilots_fit(who, *p))
        return AFT_ERR_SHAPE;
    return AFT_OK;
}

// what the multi-slot form adds to the plan's checks, in the name of the entry point that asks; 0 = fine.  group = 1,
// slots = window = 1, horizon = 0 always pass
int check_lmmse_seq(const aft_lmmse *p, int group, int slots, int window, int horizon, const char *who = "lmmse seq") {
    if (!within(who, "group", group, 1, AFT_CHANSIM_MAX_GROUP) || !within(who, "slots", slots, 1, AFT_CHANSIM_MAX_SLOTS) ||
        !within(who, "window", window, 1, slots) ||
        !within(who, "window * pilot_symbols", window * p->pilot_symbols, 1, AFT_LMMSE_MAX_WINDOW_PILOTS) ||
        !within(who, "horizon", horizon, 0, slots - 1))
        return AFT_ERR_SHAPE;
    return AFT_OK;
}

template <class... P>
bool aligned(size_t bytes, const P *...p) {
    return (... | reinterpret_cast<uintptr_t>(p)) % bytes == 0;
}

// what every link entry point asks of the struct; 0 = fine
int check_link(const char *who, const aft_link &l) {
    if (!grid_ok(who, l, INT32_MAX)) return AFT_ERR_SHAPE;
    if ((unsigned long long)l.num_scs * (unsigned long long)l.num_symbols > (1ull << 31)) {
        set_error("%s: the grid %d x %d has more than 2^31 elements", who, l.num_scs, l.num_symbols);
        return AFT_ERR_SHAPE;
    }
    if (!pilots_fit(who, l) || !pilot_index_ok(who, l, true)) return AFT_ERR_SHAPE;
    const int m = l.bits_per_symbol;
    if (m != 2 && m != 4 && m != 6 && m != 8) {
        set_error("%s: bits_per_symbol = %d is not one of 2, 4, 6, 8", who, m);
        return AFT_ERR_SHAPE;
    }
    return AFT_OK;
}

// the interleaver of the coded links: a stride in [1, used) coprime to the used bits, and its inverse
bool stride_ok(const char *who, unsigned long long stride, unsigned long long stride_inverse, unsigned long long used) {
    if (stride < 1 || stride >= used) {
        set_error("%s: stride = %llu is outside [1, %llu)", who, stride, used);
        return false;
    }
    unsigned long long g = stride, r = used;
    while (r != 0) {
        const unsigned long long next = g % r;
        g = r; r = next;
    }
    if (g != 1) {
        set_error("%s: stride = %llu is not coprime to the %llu used bits", who, stride, used);
        return false;
    }
    if (stride_inverse < 1 || stride_inverse >= used || (unsigned long long)((unsigned __int128)stride * stride_inverse % used) != 1) {
        set_error("%s: stride_inverse = %llu is not the inverse of stride = %llu modulo %llu", who, stride_inverse, stride, used);
        return false;
    }
    return true;
}

// What the three front-end entry points ask of their operands, in their order of precedence: ideal, est and keys, the `words` (4-byte
// operands that must be there, listed as `names` in the message) and llr (4-byte, may be NULL), the batch, the factors and the branches
// (an entry point without factors or branches passes 1), then the struct; 0 = fine
int check_front(const char *who, const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                std::initializer_list<const void *> words, const char *names, const float *llr, int batch, int n_factors, int branches) {
    bool there = link && ideal && est && keys;
    uintptr_t low_bits = reinterpret_cast<uintptr_t>(llr);
    for (const void *w : words) {
        there = there && w;
        low_bits |= reinterpret_cast<uintptr_t>(w);
    }
    AFT_REQUIRE(there, "%s: NULL pointer argument", who);
    AFT_REQUIRE(aligned(8, ideal, est, keys), "%s: ideal, est and keys must be 8-byte aligned", who);
    AFT_REQUIRE(low_bits % 4 == 0, "%s: %s must be 4-byte aligned", who, names);
    AFT_REQUIRE(batch >= 1, "%s: batch must be at least 1 (got %d)", who, batch);
    AFT_REQUIRE(n_factors >= 1 && n_factors <= 8, "%s: n_factors = %d is outside 1..8", who, n_factors);
    if (!within(who, "branches", branches, 1, AFT_LINK_MAX_BRANCHES)) return AFT_ERR_SHAPE;
    AFT_REQUIRE(batch % branches == 0, "%s: batch = %d is not a multiple of branches = %d", who, batch, branches);
    return check_link(who, *link);
}

// What the two two-stream entry points ask: check_front with one branch -- the group of this link is branches * streams frames --,
// then the streams, the branches and the batch against the group; 0 = fine
int check_front2(const char *who, const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                 std::initializer_list<const void *> words, const char *names, const float *llr, int batch, int n_factors, int branches,
                 int streams) {
    const int rc = check_front(who, link, ideal, est, keys, words, names, llr, batch, n_factors, 1);
    if (rc != AFT_OK) return rc;
    if (streams != AFT_LINK_MAX_STREAMS) {
        set_error("%s: streams = %d: the detector separates %d streams", who, streams, AFT_LINK_MAX_STREAMS);
        return AFT_ERR_SHAPE;
    }
    if (!within(who, "branches", branches, 2, AFT_LINK_MAX_BRANCHES)) return AFT_ERR_SHAPE;
    AFT_REQUIRE(batch % (branches * streams) == 0, "%s: batch = %d is not a multiple of branches * streams = %d * %d", who, batch,
                branches, streams);
    return AFT_OK;
}

// What the transmit-diversity entry point asks: check_front with one branch -- the group of this link is branches * 2 frames, the
// pairs (receive antenna, transmit antenna) --, then the branches, the pairing and the batch against the group; 0 = fine
int check_front_pairs(const char *who, const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                      std::initializer_list<const void *> words, const char *names, const float *llr, int batch, int n_factors,
                      int branches, int pairing) {
    const int rc = check_front(who, link, ideal, est, keys, words, names, llr, batch, n_factors, 1);
    if (rc != AFT_OK) return rc;
    if (!within(who, "branches", branches, 1, AFT_LINK_MAX_BRANCHES)) return AFT_ERR_SHAPE;
    if (pairing != AFT_LINK_PAIR_TIME && pairing != AFT_LINK_PAIR_FREQUENCY) {
        set_error("%s: pairing = %d is neither AFT_LINK_PAIR_TIME nor AFT_LINK_PAIR_FREQUENCY", who, pairing);
        return AFT_ERR_SHAPE;
    }
    AFT_REQUIRE(batch % (branches * 2) == 0, "%s: batch = %d is not a multiple of branches * 2 = %d * 2", who, batch, branches);
    return AFT_OK;
}

// What both decoder entry points compute from a block's coded and information bits and refuse: B = carried / coded blocks per frame
// (at least one; B info at most 2^31) and the interleaver's stride over the B coded used bits; 0 = fine, *blocks = B
int check_blocks(const char *who, const aft_link &l, unsigned long long coded, unsigned long long info, unsigned long long stride,
                 unsigned long long stride_inverse, unsigned *blocks) {
    const unsigned long long carried = (unsigned long long)l.bits_per_symbol *
        ((unsigned long long)l.num_scs * l.num_symbols - (unsigned long long)l.pilot_scs * l.pilot_symbols);
    const unsigned long long b = carried / coded, used = b * coded;
    if (b == 0) {
        set_error("%s: a frame carries %llu bits, fewer than the %llu coded bits of one block", who, carried, coded);
        return AFT_ERR_SHAPE;
    }
    if (b * info > (1ull << 31)) {
        set_error("%s: %llu blocks of %llu information bits: more than 2^31, where the hash's index and the int32 counts end", who, b, info);
        return AFT_ERR_SHAPE;
    }
    if (!stride_ok(who, stride, stride_inverse, used)) return AFT_ERR_SHAPE;   // used >= 10: no block has fewer coded bits
    *blocks = (unsigned)b;
    return AFT_OK;
}

// What both entry points with the QC-LDPC code ask of it: the base matrix's shape, the decoder's offset and max_iters, every shift of
// the information part (host memory), a column without an entry, the number of entries
bool ldpc_code_ok(const char *who, int base_rows, int base_cols, const int32_t *shifts, int offset, int max_iters) {
    if (!within(who, "base_rows", base_rows, 3, 16) || !within(who, "base_cols", base_cols, base_rows + 1, 32) ||
        !within(who, "offset", offset, 0, 127) || !within(who, "max_iters", max_iters, 1, 255))
        return false;
    const int kb = base_cols - base_rows;
    int edges = 3 + 2 * (base_rows - 1);                        // the parity part
    for (int j = 0; j < kb; ++j) {
        int weight = 0;
        for (int i = 0; i < base_rows; ++i) {
            const int s = shifts[i * kb + j];
            if (s < -1 || s >= AFT_LINK_LDPC_Z) {
                set_error("%s: shifts[%d][%d] = %d is neither -1 nor a shift in 0..%d", who, i, j, s, AFT_LINK_LDPC_Z - 1);
                return false;
            }
            weight += s >= 0 ? 1 : 0;
        }
        if (weight == 0) {
            set_error("%s: base column %d has no entry", who, j);
            return false;
        }
        edges += weight;
    }
    if (edges > AFT_LINK_LDPC_MAX_EDGES) {
        set_error("%s: %d entries in the base matrix, parity part included; at most %d", who, edges, AFT_LINK_LDPC_MAX_EDGES);
        return false;
    }
    return true;
}

// What both simulator entry points ask: the pointers, the batch, the group rx x tx (the ungrouped entry point passes 1 x 1 and no
// mix), the frame (group) numbers -- every FRAME number stays below 2^63 --, the struct, and a finite mix; 0 = fine.  The sequence entry
// point passes its slots (the others 1): the unit that base, start, stride and modulo count, and batch is a multiple of, is then the
// sequence of slots * rx * tx frames
int check_chansim(const char *who, const aft_chansim *sim, const float *mix, int rx, int tx, long long base, long long start,
                  long long stride, long long modulo, int batch, const float *ideal, const float *pilots, const float *meta,
                  int slots = 1) {
    AFT_REQUIRE(sim && ideal && pilots && meta, "%s: NULL pointer argument", who);
    AFT_REQUIRE(aligned(8, ideal, pilots), "%s: ideal and pilots must be 8-byte aligned", who);
    AFT_REQUIRE(aligned(4, meta, mix), "%s: %s must be 4-byte aligned", who, mix ? "meta and mix" : "meta");
    AFT_REQUIRE(batch >= 1, "%s: batch must be at least 1 (got %d)", who, batch);
    if (!within(who, "rx", rx, 1, AFT_CHANSIM_MAX_GROUP) || !within(who, "tx", tx, 1, AFT_CHANSIM_MAX_GROUP) ||
        !within(who, "rx * tx", rx * tx, 1, AFT_CHANSIM_MAX_GROUP))
        return AFT_ERR_SHAPE;
    const int group = rx * tx;
    const int unit = slots * group;                            // slots <= AFT_CHANSIM_MAX_SLOTS: checked by the caller
    if (slots == 1)
        AFT_REQUIRE(batch % group == 0, "%s: batch = %d is not a multiple of rx * tx = %d * %d", who, batch, rx, tx);
    else
        AFT_REQUIRE(batch % unit == 0, "%s: batch = %d is not a multiple of slots * rx * tx = %d * %d * %d", who, batch, slots, rx, tx);
    const long long far = (1LL << 62) / unit;
    AFT_REQUIRE(base >= 0 && start >= 0 && stride >= 1 && modulo >= 1 && base < far && modulo < far && start < far &&
                    stride <= (far - start) / (batch / unit),
                "%s: bad frame numbers (base %lld, start %lld, stride %lld, modulo %lld: base, start >= 0, stride, modulo >= 1, "
                "all frame numbers below 2^62)", who, base, start, stride, modulo);
    if (!grid_ok(who, *sim, 1 << 20) || !within(who, "taps", sim->taps, 1, AFT_CHANSIM_MAX_TAPS) ||
        !within(who, "rays", sim->rays, 1, AFT_CHANSIM_MAX_RAYS) || !within(who, "n_snr", sim->n_snr, 1, AFT_CHANSIM_MAX_VALUES) ||
        !within(who, "n_ds", sim->n_ds, 1, AFT_CHANSIM_MAX_VALUES) || !within(who, "n_dop", sim->n_dop, 1, AFT_CHANSIM_MAX_VALUES) ||
        !pilot_index_ok(who, *sim, false))
        return AFT_ERR_SHAPE;
    for (int i = 0; mix && i < group * (group + 1); ++i)
        AFT_REQUIRE(std::isfinite(mix[i]), "%s: mix[%d] = %g is not finite", who, i, (double)mix[i]);
    return AFT_OK;
}

}  // namespace

extern "C" {

int aft_channel_sim_f32(const aft_chansim *sim, unsigned long long seed, long long base, long long start, long long stride,
                        long long modulo, int batch, float *ideal, float *pilots, float *meta, void *stream) {
    const int rc = check_chansim("channel sim", sim, nullptr, 1, 1, base, start, stride, modulo, batch, ideal, pilots, meta);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_channel_sim(*sim, seed, base, start, stride, modulo, batch, ideal, pilots, meta, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("channel_sim", e);
}

int aft_channel_sim_group_f32(const aft_chansim *sim, int rx, int tx, const float *mix, unsigned long long seed, long long base,
                              long long start, long long stride, long long modulo, int batch, float *ideal, float *pilots,
                              float *meta, void *stream) {
    AFT_REQUIRE(mix, "channel sim group: NULL pointer argument");
    const int rc = check_chansim("channel sim group", sim, mix, rx, tx, base, start, stride, modulo, batch, ideal, pilots, meta);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_channel_sim_group(*sim, rx * tx, mix, seed, base, start, stride, modulo, batch, ideal, pilots, meta,
                                            static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("channel_sim_group", e);
}

// The group entry point's checks with the sequence as the unit, after the slots: slots and slots * slot_symbols within
// AFT_CHANSIM_MAX_SLOTS, slot_symbols no shorter than the grid (AFT_ERR_SHAPE, as a dimension beyond its bound)
int aft_channel_sim_seq_f32(const aft_chansim *sim, int rx, int tx, const float *mix, int slots, int slot_symbols,
                            unsigned long long seed, long long base, long long start, long long stride, long long modulo, int batch,
                            float *ideal, float *pilots, float *meta, void *stream) {
    const char *who = "channel sim seq";
    AFT_REQUIRE(mix && sim, "channel sim seq: NULL pointer argument");
    if (!within(who, "slots", slots, 1, AFT_CHANSIM_MAX_SLOTS) ||
        !within(who, "slot_symbols", slot_symbols, sim->num_symbols > 1 ? sim->num_symbols : 1, AFT_CHANSIM_MAX_SLOTS) ||
        !within(who, "slots * slot_symbols", slots * slot_symbols, 1, AFT_CHANSIM_MAX_SLOTS))
        return AFT_ERR_SHAPE;
    const int rc = check_chansim(who, sim, mix, rx, tx, base, start, stride, modulo, batch, ideal, pilots, meta, slots);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_channel_sim_seq(*sim, rx * tx, mix, slots, slot_symbols, seed, base, start, stride, modulo, batch, ideal, pilots,
                                          meta, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("channel_sim_seq", e);
}

size_t aft_lmmse_table_floats(const aft_lmmse *plan) {
    if (plan == nullptr || check_lmmse(plan) != AFT_OK) return 0;
    return (size_t)plan->n_ds * lmmse_fblock_floats(*plan) + (size_t)plan->n_dop * lmmse_tblock_floats(*plan);
}

int aft_lmmse_f32(const aft_lmmse *plan, const float *tables, const float *pilots, const float *snr, const float *ds,
                  const float *dop, float *est, int batch, void *stream) {
    AFT_REQUIRE(plan && tables && pilots && est, "lmmse: NULL pointer argument");
    AFT_REQUIRE(aligned(8, tables, pilots, est), "lmmse: tables, pilots and est must be 8-byte aligned");
    AFT_REQUIRE(aligned(4, snr, ds, dop), "lmmse: the condition arrays must be 4-byte aligned");
    AFT_REQUIRE(batch >= 1, "lmmse: batch must be at least 1 (got %d)", batch);
    const int rc = check_lmmse(plan);
    if (rc != AFT_OK) return rc;
    AFT_REQUIRE((snr || plan->fixed_snr >= 0) && (ds || plan->fixed_ds >= 0) && (dop || plan->fixed_dop >= 0),
                "lmmse: NULL condition array whose fixed_* index is -1 (snr %p / %d, ds %p / %d, dop %p / %d)", (const void *)snr,
                plan->fixed_snr, (const void *)ds, plan->fixed_ds, (const void *)dop, plan->fixed_dop);
    hipError_t e = launch_lmmse(*plan, tables, pilots, snr, ds, dop, est, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("lmmse", e);
}

size_t aft_lmmse_seq_table_floats(const aft_lmmse *plan, int window) {
    if (plan == nullptr || check_lmmse(plan) != AFT_OK || check_lmmse_seq(plan, 1, AFT_CHANSIM_MAX_SLOTS, window, 0) != AFT_OK) return 0;
    return (size_t)plan->n_ds * lmmse_fblock_floats(*plan) + (size_t)plan->n_dop * lmmse_seq_tblock_floats(*plan, window);
}

int aft_lmmse_seq_f32(const aft_lmmse *plan, int group, int slots, int window, int horizon, const float *tables, const float *pilots,
                      const float *snr, const float *ds, const float *dop, float *est, int batch, void *stream) {
    AFT_REQUIRE(plan && tables && pilots && est, "lmmse seq: NULL pointer argument");
    AFT_REQUIRE(aligned(8, tables, pilots, est), "lmmse seq: tables, pilots and est must be 8-byte aligned");
    AFT_REQUIRE(aligned(4, snr, ds, dop), "lmmse seq: the condition arrays must be 4-byte aligned");
    AFT_REQUIRE(batch >= 1, "lmmse seq: batch must be at least 1 (got %d)", batch);
    int rc = check_lmmse(plan);
    if (rc == AFT_OK) rc = check_lmmse_seq(plan, group, slots, window, horizon);
    if (rc != AFT_OK) return rc;
    AFT_REQUIRE(batch % (slots * group) == 0, "lmmse seq: batch = %d is not a multiple of slots * group = %d * %d: whole sequences only",
                batch, slots, group);
    AFT_REQUIRE((snr || plan->fixed_snr >= 0) && (ds || plan->fixed_ds >= 0) && (dop || plan->fixed_dop >= 0),
                "lmmse seq: NULL condition array whose fixed_* index is -1 (snr %p / %d, ds %p / %d, dop %p / %d)", (const void *)snr,
                plan->fixed_snr, (const void *)ds, plan->fixed_ds, (const void *)dop, plan->fixed_dop);
    hipError_t e = launch_lmmse_seq(*plan, group, slots, window, horizon, tables, pilots, snr, ds, dop, est, batch,
                                    static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("lmmse_seq", e);
}

int aft_lmmse_grid_f32(const aft_lmmse *plan, int kf, const float *tables, const float *z, const float *snr, const float *ds,
                       const float *dop, float *est, int batch, void *stream) {
    const char *who = "lmmse grid";
    AFT_REQUIRE(plan && tables && z && est, "lmmse grid: NULL pointer argument");
    AFT_REQUIRE(aligned(8, tables, z, est), "lmmse grid: tables, z and est must be 8-byte aligned");
    AFT_REQUIRE(aligned(4, snr, ds, dop), "lmmse grid: the condition arrays must be 4-byte aligned");
    AFT_REQUIRE(batch >= 1, "lmmse grid: batch must be at least 1 (got %d)", batch);
    const int rc = check_lmmse(plan);
    if (rc != AFT_OK) return rc;
    if (plan->num_symbols > AFT_LMMSE_MAX_WINDOW_PILOTS) {
        set_error("lmmse grid: num_symbols = %d: the full-grid smoother filters all T symbols of a frame at once and holds at most "
                  "AFT_LMMSE_MAX_WINDOW_PILOTS = %d of them", plan->num_symbols, AFT_LMMSE_MAX_WINDOW_PILOTS);
        return AFT_ERR_SHAPE;
    }
    if (!within(who, "kf", kf, 1, plan->num_scs < AFT_CHANSIM_MAX_TAPS ? plan->num_scs : AFT_CHANSIM_MAX_TAPS)) return AFT_ERR_SHAPE;
    AFT_REQUIRE((snr || plan->fixed_snr >= 0) && (ds || plan->fixed_ds >= 0) && (dop || plan->fixed_dop >= 0),
                "lmmse grid: NULL condition array whose fixed_* index is -1 (snr %p / %d, ds %p / %d, dop %p / %d)", (const void *)snr,
                plan->fixed_snr, (const void *)ds, plan->fixed_ds, (const void *)dop, plan->fixed_dop);
    hipError_t e = launch_lmmse_grid(*plan, kf, tables, z, snr, ds, dop, est, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("lmmse_grid", e);
}

size_t aft_lmmse_classify_table_floats(const aft_lmmse *plan, int window) {
    if (plan == nullptr || check_lmmse(plan) != AFT_OK ||
        check_lmmse_seq(plan, 1, AFT_CHANSIM_MAX_SLOTS, window, 0, "lmmse classify") != AFT_OK)
        return 0;
    return lmmse_classify_table_floats(*plan, window);
}

int aft_lmmse_classify_f32(const aft_lmmse *plan, int group, int slots, int window, int horizon, int pool, const float *tables,
                           const float *logdet, const float *pilots, int32_t *idx, float *snr, float *ds, float *dop, float *scores,
                           int batch, void *stream) {
    AFT_REQUIRE(plan && tables && logdet && pilots && idx && snr && ds && dop, "lmmse classify: NULL pointer argument (only scores may be NULL)");
    AFT_REQUIRE(aligned(8, tables, pilots), "lmmse classify: tables and pilots must be 8-byte aligned");
    AFT_REQUIRE(aligned(4, logdet, snr, ds, dop, scores) && aligned(4, idx), "lmmse classify: logdet, idx, snr, ds, dop and scores must be 4-byte aligned");
    AFT_REQUIRE(batch >= 1, "lmmse classify: batch must be at least 1 (got %d)", batch);
    AFT_REQUIRE(pool == 0 || pool == 1, "lmmse classify: pool must be 0 (a frame decides alone) or 1 (a group decides together), got %d", pool);
    int rc = check_lmmse(plan);
    if (rc == AFT_OK) rc = check_lmmse_seq(plan, group, slots, window, horizon, "lmmse classify");
    if (rc != AFT_OK) return rc;
    AFT_REQUIRE(batch % (slots * group) == 0, "lmmse classify: batch = %d is not a multiple of slots * group = %d * %d: whole sequences only",
                batch, slots, group);
    hipError_t e = launch_lmmse_classify(*plan, group, slots, window, horizon, pool, tables, logdet, pilots, idx, snr, ds, dop, scores,
                                         batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("lmmse_classify", e);
}

int aft_link_errors_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                        const float *sigma, int32_t *counts, int batch, void *stream) {
    const int rc = check_front("link errors", link, ideal, est, keys, {sigma, counts}, "sigma and counts", nullptr, batch, 1, 1);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_link_errors(*link, ideal, est, keys, sigma, counts, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_errors", e);
}

int aft_link_soft_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                      const float *sigma, const float *scale, const float *factors, int n_factors, float *loss, float *llr,
                      int batch, void *stream) {
    const int rc = check_front("link soft", link, ideal, est, keys, {sigma, scale, factors, loss}, "sigma, scale, factors, loss and llr", llr,
                               batch, n_factors, 1);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_link_soft(*link, ideal, est, keys, sigma, scale, factors, n_factors, loss, llr, batch,
                                    static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_soft", e);
}

int aft_link_decode_f32(const aft_link *link, const float *llr, const unsigned long long *keys, int info_bits, int rate,
                        unsigned long long stride, unsigned long long stride_inverse, float qgain, int32_t *counts,
                        unsigned char *bits, int batch, void *stream) {
    const char *who = "link decode";
    AFT_REQUIRE(link && llr && keys && counts, "link decode: NULL pointer argument");
    AFT_REQUIRE(aligned(8, keys), "link decode: keys must be 8-byte aligned");
    AFT_REQUIRE(aligned(4, llr, counts), "link decode: llr and counts must be 4-byte aligned");
    AFT_REQUIRE(batch >= 1, "link decode: batch must be at least 1 (got %d)", batch);
    AFT_REQUIRE(std::isfinite(qgain) && qgain > 0.f, "link decode: qgain = %g must be finite and positive", (double)qgain);
    const int rc = check_link(who, *link);
    if (rc != AFT_OK) return rc;
    if (!within(who, "info_bits", info_bits, 1, AFT_LINK_CODE_MAX_INFO_BITS)) return AFT_ERR_SHAPE;
    if (rate != AFT_LINK_RATE_1_2 && rate != AFT_LINK_RATE_2_3 && rate != AFT_LINK_RATE_3_4) {
        set_error("%s: rate = %d is not one of AFT_LINK_RATE_1_2, _2_3, _3_4", who, rate);
        return AFT_ERR_SHAPE;
    }
    // kept outputs of the K + 6 steps: A0 B0 | A0 B0 A1 | A0 B0 A1 B2 per period of 1, 2, 3 steps
    const unsigned long long steps = (unsigned long long)info_bits + 6;
    const unsigned long long coded = rate == AFT_LINK_RATE_1_2   ? 2 * steps
                                     : rate == AFT_LINK_RATE_2_3 ? 3 * (steps / 2) + 2 * (steps % 2)
                                                                 : 4 * (steps / 3) + (steps % 3 == 0 ? 0 : steps % 3 + 1);
    unsigned blocks = 0;
    const int rb = check_blocks(who, *link, coded, (unsigned long long)info_bits, stride, stride_inverse, &blocks);
    if (rb != AFT_OK) return rb;
    hipError_t e = launch_link_decode(*link, llr, keys, info_bits, rate, (unsigned)coded, blocks, stride, qgain,
                                      counts, bits, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_decode", e);
}

// What both LDPC decoder entry points do after their own operands: aft_link_ldpc_f32's checks under the caller's name, then the launch --
// the masked kernel where mask is given (aft_link_ldpc_masked_f32 has checked it and its stride)
static int link_ldpc_checked(const char *who, const char *what, const aft_link *link, const float *llr, const unsigned long long *keys,
                             int base_rows, int base_cols, const int32_t *shifts, unsigned long long stride,
                             unsigned long long stride_inverse, float qgain, int offset, int max_iters, int32_t *counts, unsigned char *bits,
                             const int32_t *mask, int mask_stride, int batch, void *stream) {
    AFT_REQUIRE(link && llr && keys && shifts && counts, "%s: NULL pointer argument", who);
    AFT_REQUIRE(aligned(8, keys), "%s: keys must be 8-byte aligned", who);
    AFT_REQUIRE(aligned(4, llr, shifts, counts), "%s: llr, shifts and counts must be 4-byte aligned", who);
    AFT_REQUIRE(batch >= 1, "%s: batch must be at least 1 (got %d)", who, batch);
    AFT_REQUIRE(std::isfinite(qgain) && qgain > 0.f, "%s: qgain = %g must be finite and positive", who, (double)qgain);
    const int rc = check_link(who, *link);
    if (rc != AFT_OK) return rc;
    if (!ldpc_code_ok(who, base_rows, base_cols, shifts, offset, max_iters)) return AFT_ERR_SHAPE;
    const int kb = base_cols - base_rows;
    const unsigned long long coded = (unsigned long long)base_cols * AFT_LINK_LDPC_Z, info = (unsigned long long)kb * AFT_LINK_LDPC_Z;
    unsigned blocks = 0;
    const int rb = check_blocks(who, *link, coded, info, stride, stride_inverse, &blocks);
    if (rb != AFT_OK) return rb;
    hipError_t e = launch_link_ldpc(*link, llr, keys, base_rows, base_cols, shifts, blocks, stride, qgain, offset, max_iters,
                                    counts, bits, mask, mask_stride, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail(what, e);
}

int aft_link_ldpc_f32(const aft_link *link, const float *llr, const unsigned long long *keys, int base_rows, int base_cols,
                      const int32_t *shifts, unsigned long long stride, unsigned long long stride_inverse, float qgain, int offset,
                      int max_iters, int32_t *counts, unsigned char *bits, int batch, void *stream) {
    return link_ldpc_checked("link ldpc", "link_ldpc", link, llr, keys, base_rows, base_cols, shifts, stride, stride_inverse, qgain, offset,
                             max_iters, counts, bits, nullptr, 0, batch, stream);
}

// aft_link_ldpc_f32's checks after its own: the mask is there, 4-byte aligned, and read at a stride of at least one word
int aft_link_ldpc_masked_f32(const aft_link *link, const float *llr, const unsigned long long *keys, int base_rows, int base_cols,
                             const int32_t *shifts, unsigned long long stride, unsigned long long stride_inverse, float qgain, int offset,
                             int max_iters, const int32_t *mask, int mask_stride, int32_t *counts, unsigned char *bits, int batch,
                             void *stream) {
    AFT_REQUIRE(mask, "link ldpc masked: NULL pointer argument");
    AFT_REQUIRE(aligned(4, mask), "link ldpc masked: mask must be 4-byte aligned");
    AFT_REQUIRE(mask_stride >= 1, "link ldpc masked: mask_stride must be at least 1 (got %d)", mask_stride);
    return link_ldpc_checked("link ldpc masked", "link_ldpc_masked", link, llr, keys, base_rows, base_cols, shifts, stride, stride_inverse,
                             qgain, offset, max_iters, counts, bits, mask, mask_stride, batch, stream);
}

int aft_link_mrc_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                     const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors, int branches,
                     int32_t *counts, float *loss, float *llr, int batch, void *stream) {
    const int rc = check_front("link mrc", link, ideal, est, keys, {sigma, rho, scale, factors, counts, loss},
                               "sigma, rho, scale, factors, counts, loss and llr", llr, batch, n_factors, branches);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_link_mrc(*link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, counts, loss, llr, batch,
                                   static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_mrc", e);
}

int aft_link_observe_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                         const float *sigma, const float *rho, const float *pilots, int source, int branches, float *z,
                         unsigned char *decisions, int32_t *symbol_errors, int batch, void *stream) {
    const int rc = check_front("link observe", link, ideal, est, keys, {sigma, rho, symbol_errors}, "sigma, rho and symbol_errors", nullptr,
                               batch, 1, branches);
    if (rc != AFT_OK) return rc;
    AFT_REQUIRE(pilots && z && decisions, "link observe: NULL pointer argument");
    AFT_REQUIRE(aligned(8, pilots, z), "link observe: pilots and z must be 8-byte aligned");
    AFT_REQUIRE(source == AFT_LINK_OBSERVE_DECIDED || source == AFT_LINK_OBSERVE_SENT,
                "link observe: source = %d is neither AFT_LINK_OBSERVE_DECIDED nor AFT_LINK_OBSERVE_SENT", source);
    hipError_t e = launch_link_observe(*link, ideal, est, keys, sigma, rho, pilots, source, branches, z, decisions, symbol_errors, batch,
                                       static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_observe", e);
}

int aft_link_harq_f32(const aft_link *link, const float *llr, const unsigned long long *keys, int base_rows, int base_cols,
                      const int32_t *shifts, int tx_cols, int rounds, const int32_t *starts, unsigned long long stride,
                      unsigned long long stride_inverse, float qgain, int offset, int max_iters, int32_t *counts, unsigned char *bits,
                      int batch, void *stream) {
    const char *who = "link harq";
    AFT_REQUIRE(link && llr && keys && shifts && starts && counts, "link harq: NULL pointer argument");
    AFT_REQUIRE(aligned(8, keys), "link harq: keys must be 8-byte aligned");
    AFT_REQUIRE(aligned(4, llr, shifts, starts, counts), "link harq: llr, shifts, starts and counts must be 4-byte aligned");
    AFT_REQUIRE(batch >= 1, "link harq: batch must be at least 1 (got %d)", batch);
    AFT_REQUIRE(std::isfinite(qgain) && qgain > 0.f, "link harq: qgain = %g must be finite and positive", (double)qgain);
    const int rc = check_link(who, *link);
    if (rc != AFT_OK) return rc;
    if (!within(who, "rounds", rounds, 1, AFT_LINK_HARQ_MAX_ROUNDS)) return AFT_ERR_SHAPE;
    AFT_REQUIRE(batch % rounds == 0, "link harq: batch = %d is not a multiple of rounds = %d", batch, rounds);
    if (!ldpc_code_ok(who, base_rows, base_cols, shifts, offset, max_iters)) return AFT_ERR_SHAPE;
    const int kb = base_cols - base_rows;
    if (!within(who, "tx_cols", tx_cols, kb + 1, base_cols)) return AFT_ERR_SHAPE;
    for (int t = 0; t < rounds; ++t) {
        if (starts[t] >= 0 && starts[t] < base_cols) continue;
        set_error("%s: starts[%d] = %d is outside 0..%d", who, t, starts[t], base_cols - 1);
        return AFT_ERR_SHAPE;
    }
    // a round's tx_cols block columns are what a block occupies on the link: B, U and the stride follow from them
    const unsigned long long sent = (unsigned long long)tx_cols * AFT_LINK_LDPC_Z, info = (unsigned long long)kb * AFT_LINK_LDPC_Z;
    unsigned blocks = 0;
    const int rb = check_blocks(who, *link, sent, info, stride, stride_inverse, &blocks);
    if (rb != AFT_OK) return rb;
    hipError_t e = launch_link_harq(*link, llr, keys, base_rows, base_cols, shifts, tx_cols, rounds, starts, blocks, stride, qgain, offset,
                                    max_iters, counts, bits, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_harq", e);
}

int aft_link_sm_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys, const float *sigma,
                    const float *rho, const float *scale, const float *reg, const float *factors, int n_factors, int branches,
                    int streams, int32_t *counts, float *loss, float *llr, int batch, void *stream) {
    const int rc = check_front2("link sm", link, ideal, est, keys, {sigma, rho, scale, reg, factors, counts, loss},
                                "sigma, rho, scale, reg, factors, counts, loss and llr", llr, batch, n_factors, branches, streams);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_link2(false, *link, ideal, est, keys, sigma, rho, scale, reg, factors, n_factors, branches, counts, loss, llr,
                                batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_sm", e);
}

int aft_link_joint_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys, const float *sigma,
                       const float *rho, const float *scale, const float *factors, int n_factors, int branches, int streams,
                       int32_t *counts, float *loss, float *llr, int batch, void *stream) {
    const int rc = check_front2("link joint", link, ideal, est, keys, {sigma, rho, scale, factors, counts, loss},
                                "sigma, rho, scale, factors, counts, loss and llr", llr, batch, n_factors, branches, streams);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_link2(true, *link, ideal, est, keys, sigma, rho, scale, nullptr, factors, n_factors, branches, counts, loss, llr,
                                batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_joint", e);
}

// aft_link_sm_f32's checks; stats may be NULL as llr may, and is 4-byte aligned where it is given
int aft_link_sic_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys, const float *sigma,
                     const float *rho, const float *scale, const float *reg, const float *factors, int n_factors, int branches,
                     int streams, int32_t *counts, float *loss, float *llr, int32_t *stats, int batch, void *stream) {
    const int rc = check_front2("link sic", link, ideal, est, keys, {sigma, rho, scale, reg, factors, counts, loss},
                                "sigma, rho, scale, reg, factors, counts, loss, llr and stats", llr, batch, n_factors, branches, streams);
    if (rc != AFT_OK) return rc;
    AFT_REQUIRE(aligned(4, stats), "link sic: sigma, rho, scale, reg, factors, counts, loss, llr and stats must be 4-byte aligned");
    hipError_t e = launch_link_sic(*link, ideal, est, keys, sigma, rho, scale, reg, factors, n_factors, branches, counts, loss, llr, stats,
                                   batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_sic", e);
}

// aft_link_sm_f32's checks less reg; failed is there, 4-byte aligned and read at a stride of at least one word; state may be NULL as llr
// may, and is 4-byte aligned where it is given
int aft_link_cancel_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys, const float *sigma,
                        const float *rho, const float *scale, const float *factors, int n_factors, int branches, int streams,
                        const int32_t *failed, int failed_stride, int32_t *counts, float *loss, float *llr, int32_t *state, int batch,
                        void *stream) {
    const int rc = check_front2("link cancel", link, ideal, est, keys, {sigma, rho, scale, factors, failed, counts, loss},
                                "sigma, rho, scale, factors, failed, counts, loss, llr and state", llr, batch, n_factors, branches, streams);
    if (rc != AFT_OK) return rc;
    AFT_REQUIRE(aligned(4, state), "link cancel: sigma, rho, scale, factors, failed, counts, loss, llr and state must be 4-byte aligned");
    AFT_REQUIRE(failed_stride >= 1, "link cancel: failed_stride must be at least 1 (got %d)", failed_stride);
    hipError_t e = launch_link_cancel(*link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, failed, failed_stride, counts,
                                      loss, llr, state, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_cancel", e);
}

int aft_link_alamouti_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys, const float *sigma,
                          const float *rho, const float *scale, const float *factors, int n_factors, int branches, int pairing,
                          int32_t *counts, float *loss, float *llr, int batch, void *stream) {
    const int rc = check_front_pairs("link alamouti", link, ideal, est, keys, {sigma, rho, scale, factors, counts, loss},
                                     "sigma, rho, scale, factors, counts, loss and llr", llr, batch, n_factors, branches, pairing);
    if (rc != AFT_OK) return rc;
    hipError_t e = launch_link_alamouti(*link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, pairing, counts, loss,
                                        llr, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_alamouti", e);
}

// Every refusal of this entry point is AFT_ERR_ARG, the struct's included: check_front with one branch -- the group of this link is
// branches * 2 frames --, then the branches, the batch against the group and the subbands against the grid
int aft_link_precoded_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys, const float *sigma,
                          const float *rho, const float *scale, const float *factors, int n_factors, int branches, int subband,
                          int32_t *counts, float *loss, float *llr, int32_t *pmi, int batch, void *stream) {
    const char *who = "link precoded";
    if (check_front(who, link, ideal, est, keys, {sigma, rho, scale, factors, counts, loss, pmi},
                    "sigma, rho, scale, factors, counts, loss, pmi and llr", llr, batch, n_factors, 1) != AFT_OK)
        return AFT_ERR_ARG;
    if (!within(who, "branches", branches, 1, AFT_LINK_MAX_BRANCHES)) return AFT_ERR_ARG;
    AFT_REQUIRE(batch % (branches * 2) == 0, "%s: batch = %d is not a multiple of branches * 2 = %d * 2", who, batch, branches);
    if (!within(who, "subband", subband, 1, link->num_scs)) return AFT_ERR_ARG;
    const int n_sub = (link->num_scs - 1) / subband + 1;
    AFT_REQUIRE(n_sub <= AFT_LINK_MAX_SUBBANDS, "%s: subband = %d makes %d subbands of the %d subcarriers, more than %d", who, subband,
                n_sub, link->num_scs, AFT_LINK_MAX_SUBBANDS);
    hipError_t e = launch_link_precoded(*link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, subband, counts, loss,
                                        llr, pmi, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_precoded", e);
}

// aft_link_precoded_f32's refusals, then the slots, the delay and the batch against the sequence of slots * branches * 2 frames
int aft_link_precoded_delayed_f32(const aft_link *link, const float *ideal, const float *est, const unsigned long long *keys,
                                  const float *sigma, const float *rho, const float *scale, const float *factors, int n_factors,
                                  int branches, int subband, int slots, int delay, int32_t *counts, float *loss, float *llr,
                                  int32_t *pmi, int batch, void *stream) {
    const char *who = "link precoded delayed";
    if (check_front(who, link, ideal, est, keys, {sigma, rho, scale, factors, counts, loss, pmi},
                    "sigma, rho, scale, factors, counts, loss, pmi and llr", llr, batch, n_factors, 1) != AFT_OK)
        return AFT_ERR_ARG;
    if (!within(who, "branches", branches, 1, AFT_LINK_MAX_BRANCHES)) return AFT_ERR_ARG;
    AFT_REQUIRE(batch % (branches * 2) == 0, "%s: batch = %d is not a multiple of branches * 2 = %d * 2", who, batch, branches);
    if (!within(who, "subband", subband, 1, link->num_scs)) return AFT_ERR_ARG;
    const int n_sub = (link->num_scs - 1) / subband + 1;
    AFT_REQUIRE(n_sub <= AFT_LINK_MAX_SUBBANDS, "%s: subband = %d makes %d subbands of the %d subcarriers, more than %d", who, subband,
                n_sub, link->num_scs, AFT_LINK_MAX_SUBBANDS);
    AFT_REQUIRE(slots >= 1, "%s: slots must be at least 1 (got %d)", who, slots);
    AFT_REQUIRE(delay >= 0 && delay < slots, "%s: delay = %d is outside 0 .. slots - 1 = %d", who, delay, slots - 1);
    AFT_REQUIRE((batch / (branches * 2)) % slots == 0, "%s: batch = %d is not a multiple of slots * 2 * branches = %d * 2 * %d", who, batch,
                slots, branches);
    hipError_t e = launch_link_precoded_delayed(*link, ideal, est, keys, sigma, rho, scale, factors, n_factors, branches, subband, slots,
                                                delay, counts, loss, llr, pmi, batch, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? AFT_OK : hip_fail("link_precoded_delayed", e);
}

}  // extern "C"
