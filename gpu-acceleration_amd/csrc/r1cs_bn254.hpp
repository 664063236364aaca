// r1cs_bn254.hpp -- rows of R1CS constraint matrices times a witness over the BN254 scalar field: a = A w, b = B w, c = C w, the evaluations the
// Groth16 H recipes start from.  The upload plan (host), the per-item and fold routines (__host__ __device__) and the kernels that run them.
// tools/r1cs_check.cpp runs the SAME plan and routines on the CPU, item by item, under -DFP_BOUNDS_CHECK.
//
// Forms (fr_bn254.hpp: raw / rep).  A general coefficient c is kept as rep(c) = c * 2^261 mod r, canonical; the witness words are read as raw limbs,
// so fr_mul(raw(w), rep(c)) = raw(c w): a row's sum comes out in the form of the WITNESS words, whatever that is, and the change of form between
// witness and output is the one multiplication by rep(1), rep(2^256) or rep(2^-256) that also reduces the sum -- per row, not per entry.  The form
// of the coefficients as handed in (plain, * 2^256, * 2^512) only selects the constant applied once per distinct value at upload.
//
// Entries.  Almost every coefficient of a real circuit is 1 or -1, so an entry is 8 bytes: the column and a KIND -- +1, -1, or 2 + the index into
// the table of distinct other values.  +1 is a limb-wise addition of the raw witness word, -1 the padded subtraction fr_sub<7>.
//
// Work items.  Rows are cut on the host into items of at most R1CS_ITEM_LEN entries (most rows have one to three entries, a few have thousands);
// one lane runs one item.  A row that is one item writes its output directly; the items of a longer row write canonical partial sums, which
// k_r1cs_fold adds up, one wavefront per such row.  A row without entries, in a matrix that has any, is an item of length 0.  Items keep the order
// (matrix, row); 64 consecutive items form a group whose entries are stored entry-major: entry j of lane l at (group base + j) * 64 + l, so the 64
// lanes of a wavefront read 512 contiguous bytes per step.  A group is as wide as its longest item; slots beyond an item's length are never read.
//
// THE BOUND.  Nine 29-bit limbs hold values below 2^261, and 169 r < 2^261 < 170 r.  A raw witness word is any 256-bit pattern: < 2^256 < 5.3 r.
// One entry adds to the lazily reduced accumulator at most
//     +1:       w                    < 6 r
//     -1:       7 r - w              <= 7 r          (FR29_PAD[7] covers a subtrahend < 6 r)
//     general:  fr_mul(w, rep(c))    < 5.3 r * r / 2^261 + r < 2 r
// so an item of R1CS_ITEM_LEN = 24 entries stays below 24 * 7 r = 168 r < 2^261 with no reduction inside it.  The fold adds canonical partials
// (< r each): R1CS_FOLD_CHUNK = 160 of them on top of a value < 2 r stay below 162 r, then one multiplication by rep(1) brings the sum back
// below 2 r.  Every one of these is asserted under -DFP_BOUNDS_CHECK, in units of r (R1CS_ACC_MAX_R) and limb by limb (fr_normalize).
#pragma once
#include "ntt_bn254.hpp"

#include <array>
#include <string>
#include <unordered_map>
#include <vector>

namespace r1csk {

using namespace nttk;

constexpr uint32_t R1CS_ITEM_LEN = 24;     // entries per work item
constexpr uint32_t R1CS_ACC_MAX_R = 168;   // the accumulator may hold values < 168 r + r <= 169 r < 2^261
constexpr uint32_t R1CS_FOLD_CHUNK = 160;  // partials added between two reductions of the fold
constexpr uint32_t R1CS_GROUP = 64;        // items per group: one wavefront
constexpr uint32_t R1CS_ITEM_PARTIAL = 0x80000000u;
constexpr uint32_t R1CS_KIND_PLUS = 0, R1CS_KIND_MINUS = 1, R1CS_KIND_DICT = 2;
constexpr uint32_t R1CS_COEF_STD = 0, R1CS_COEF_MONT = 1, R1CS_COEF_MONT2 = 2;  // == MSM_R1CS_COEF_* of include/msm_hip.h
constexpr uint32_t R1CS_F_C_FROM_AB = 8;                                         // == MSM_R1CS_C_FROM_AB
static_assert(R1CS_ITEM_LEN * 7 <= R1CS_ACC_MAX_R, "an item of -1 entries must fit the accumulator");
static_assert(R1CS_FOLD_CHUNK + 2 <= R1CS_ACC_MAX_R && R1CS_GROUP <= R1CS_ACC_MAX_R, "a fold chunk must fit the accumulator");
static_assert(FR29_MAX_PAD >= 7, "the -1 entries subtract a raw 256-bit word (< 6 r) from a 7 r pad");

struct R1csCoef {  // == msm_r1cs_coef_t: one entry of a zkey's coefficient section
    uint32_t matrix, row, col;
    uint32_t value[8];
};
static_assert(sizeof(R1csCoef) == 44, "a coefficient record is 44 bytes");

struct R1csInfo {  // == msm_r1cs_info_t
    uint64_t entries[3], rows_with_entries[3];
    uint64_t longest_row, plus_one, minus_one, distinct_values;
    uint64_t work_items, max_item_len, fold_rows, partial_sums, device_bytes;
    double build_ms, upload_ms;
};

struct R1csView {
    const uint2* items;          // x = where the result goes (matrix * n + row, or the partial's slot), y = length | R1CS_ITEM_PARTIAL
    const uint32_t* group_base;  // per group of 64 items: its first entry step (units of 64 entries)
    const uint2* entries;        // x = column, y = kind
    const uint32_t* dict;        // the distinct general coefficients: rep(c), canonical, 8 words each
    const uint4* folds;          // per row of several items: x = matrix * n + row, y = its first partial, z = their number
};

// ---- one work item ------------------------------------------------------------------------------------------------------------------------
// post: rep(1), rep(2^256) or rep(2^-256), canonical: the change of form between witness and output (partials are kept in the witness' form)
NTT_HD void r1cs_item(const R1csView& v, uint32_t item, const uint32_t* wit, const fr& post, uint32_t* out, uint32_t* partials) {
    const uint2 it = v.items[item];
    const uint32_t len = it.y & ~R1CS_ITEM_PARTIAL;
    const uint2* e = v.entries + (((size_t)v.group_base[item / R1CS_GROUP]) * R1CS_GROUP + item % R1CS_GROUP);
    fr acc = fr_zero();
    uint32_t bound = 0;  // acc < bound * r
    FP_ASSERT(len <= R1CS_ITEM_LEN, "r1cs item longer than R1CS_ITEM_LEN");
    for (uint32_t j = 0; j < len; j++) {
        const uint2 en = e[(size_t)j * R1CS_GROUP];
        const fr w = ntt_table(wit, en.x);  // any 256-bit pattern: normalised, < 5.3 r
        if (en.y == R1CS_KIND_PLUS) {
            acc = fr_add(acc, w);
            bound += 6;
        } else if (en.y == R1CS_KIND_MINUS) {
            acc = fr_sub<7>(acc, w);
            bound += 7;
        } else {
            acc = fr_add(acc, fr_mul(w, ntt_table(v.dict, en.y - R1CS_KIND_DICT)));  // < 5.3 r * r / 2^261 + r < 2 r
            bound += 2;
        }
        FP_ASSERT(bound <= R1CS_ACC_MAX_R, "r1cs item: the lazy sum leaves 168 r");
    }
    (void)bound;
    const bool partial = it.y & R1CS_ITEM_PARTIAL;
    // acc < 168 r, the factor < r: product < 168 r * r / 2^261 + r < 2 r.  (fr_mul needs A * B < (2^261 - r) * 2^261: 168 r < 2^261 - r ~ 168.28 r,
    // so this accumulator is inside it against ANY normalised factor -- R1CS_ACC_MAX_R may not grow past 168)
    uint32_t w8[8];
    fr_pack(w8, fr_reduce_lt2r(fr_mul(acc, partial ? fr_one() : post)));
    ntt_store8((partial ? partials : out) + (size_t)it.x * 8, w8);
}

// ---- the fold of a row of several items: lane l of 64 adds partials l, l + 64, ...; then one lane adds the 64 lane sums -----------------------
NTT_HD fr r1cs_fold_lane(const uint32_t* partials, uint32_t first, uint32_t count, uint32_t lane) {
    fr acc = fr_zero();
    uint32_t pending = 0;  // acc < (2 + pending) r
    for (uint32_t t = lane; t < count; t += R1CS_GROUP) {
        acc = fr_add(acc, ntt_table(partials, first + t));  // canonical: < r
        if (++pending == R1CS_FOLD_CHUNK) {
            acc = fr_mul(acc, fr_one());  // < 162 r * r / 2^261 + r < 2 r, the same value modulo r
            pending = 0;
        }
    }
    return fr_reduce_lt2r(fr_mul(acc, fr_one()));
}
// sums: 64 x 9 limbs, each canonical (< r): their sum < 64 r; times post < 2 r
NTT_HD void r1cs_fold_finish(const uint32_t* sums, const fr& post, uint32_t* out) {
    fr acc = fr_zero();
    for (uint32_t l = 0; l < R1CS_GROUP; l++) acc = fr_add(acc, ntt_lds_get(sums, l));
    uint32_t w8[8];
    fr_pack(w8, fr_reduce_lt2r(fr_mul(acc, post)));
    ntt_store8(out, w8);
}

inline fr r1cs_post(uint32_t flags) {
    const bool im = flags & NTT_F_IN_MONT, om = flags & NTT_F_OUT_MONT;
    return fr_canonical(om == im ? fr_one() : (om ? ntt_consts().p256 : ntt_consts().m256));
}

// ---- the host's share: validation, one counting sort by (matrix, row), the dictionary, the items and their layout ----------------------------
struct R1csHost {
    std::vector<uint2> items, entries;
    std::vector<uint32_t> group_base, dict;
    std::vector<uint4> folds;
    uint32_t items01 = 0, folds01 = 0;  // how many of them belong to matrices 0 and 1 (they come first): what MSM_R1CS_C_FROM_AB runs
    uint32_t num_rows = 0, num_cols = 0, log_n = 0;
    R1csInfo info{};
};

struct R1csKeyHash {
    size_t operator()(const std::array<uint32_t, 8>& k) const {
        uint64_t h = 1469598103934665603ull;
        for (uint32_t w : k) h = (h ^ w) * 1099511628211ull;
        return (size_t)h;
    }
};

// 0 = fine, -1 = empty, -2 = bad argument (err says which).  layout = false stops after the counts (no entry array is built).
inline int r1cs_build(const R1csCoef* coefs, size_t n_coefs, uint32_t form, uint32_t num_rows, uint32_t num_cols, uint32_t log_n, bool layout,
                      R1csHost& h, std::string& err) {
    char msg[200];
    auto bad = [&](int code) {
        err = msg;
        return code;
    };
    h = R1csHost{};
    if (n_coefs == 0) return snprintf(msg, sizeof msg, "Empty input"), bad(-1);
    if (!coefs) return snprintf(msg, sizeof msg, "NULL coefficient pointer"), bad(-2);
    if (log_n > NTT_MAX_LOG2) return snprintf(msg, sizeof msg, "log_n = %u: r - 1 has 28 factors of two", log_n), bad(-2);
    if (num_rows > (1u << log_n)) return snprintf(msg, sizeof msg, "num_rows = %u exceeds the domain 2^%u", num_rows, log_n), bad(-2);
    if (form > R1CS_COEF_MONT2) return snprintf(msg, sizeof msg, "coef_form = %u: MSM_R1CS_COEF_STD, _MONT or _MONT2", form), bad(-2);
    if (n_coefs >= 0xFFFFFFFFull) return snprintf(msg, sizeof msg, "n_coefs = %zu: at most 2^32 - 2 entries", n_coefs), bad(-2);
    const size_t nkeys = (size_t)3 * num_rows;
    std::vector<uint32_t> start(nkeys + 1, 0);
    for (size_t i = 0; i < n_coefs; i++) {
        const R1csCoef& c = coefs[i];
        if (c.matrix > 2) return snprintf(msg, sizeof msg, "entry %zu: matrix = %u (0, 1 or 2)", i, c.matrix), bad(-2);
        if (c.row >= num_rows) return snprintf(msg, sizeof msg, "entry %zu: row = %u, num_rows = %u", i, c.row, num_rows), bad(-2);
        if (c.col >= num_cols) return snprintf(msg, sizeof msg, "entry %zu: col = %u, num_cols = %u", i, c.col, num_cols), bad(-2);
        start[(size_t)c.matrix * num_rows + c.row + 1]++;
        h.info.entries[c.matrix]++;
    }
    h.num_rows = num_rows, h.num_cols = num_cols, h.log_n = log_n;
    R1csInfo& info = h.info;
    for (size_t k = 0; k < nkeys; k++) {
        const uint32_t cnt = start[k + 1];
        if (cnt) info.rows_with_entries[k / num_rows]++;
        if (cnt > info.longest_row) info.longest_row = cnt;
        start[k + 1] += start[k];
    }

    // kinds: the two common values are recognised by their words; everything else goes through the field
    const NttConsts& K = ntt_consts();
    const fr one_f = form == R1CS_COEF_STD ? fr_one() : (form == R1CS_COEF_MONT ? K.p256 : fr_mul(K.p256, K.p256));   // rep(2^(256 form))
    const fr to_rep = fr_canonical(form == R1CS_COEF_STD ? K.p261 : (form == R1CS_COEF_MONT ? K.p5 : fr_mul(K.p5, K.m256)));  // rep(2^(261 - 256 form))
    const fr rep_one = fr_canonical(fr_one()), rep_minus = fr_canonical(fr_sub<3>(fr_zero(), fr_one()));
    uint32_t w_one[8], w_minus[8];
    fr_to_std(w_one, one_f);
    fr_to_std(w_minus, fr_sub<3>(fr_zero(), one_f));
    auto same = [](const fr& a, const fr& b) {
        uint32_t d = 0;
        for (int i = 0; i < 9; i++) d |= a.v[i] ^ b.v[i];
        return d == 0;
    };
    std::unordered_map<std::array<uint32_t, 8>, uint32_t, R1csKeyHash> index;
    std::vector<uint32_t> kind(n_coefs);
    for (size_t i = 0; i < n_coefs; i++) {
        const uint32_t* v = coefs[i].value;
        uint32_t k;
        if (memcmp(v, w_one, 32) == 0) k = R1CS_KIND_PLUS;
        else if (memcmp(v, w_minus, 32) == 0) k = R1CS_KIND_MINUS;
        else {
            const fr rc = fr_reduce_lt2r(fr_mul(fr_unpack(v), to_rep));  // any pattern (< 5.3 r) times a canonical factor: < 2 r
            if (same(rc, rep_one)) k = R1CS_KIND_PLUS;
            else if (same(rc, rep_minus)) k = R1CS_KIND_MINUS;
            else {
                std::array<uint32_t, 8> key;
                fr_pack(key.data(), rc);
                auto it = index.find(key);
                if (it == index.end()) {
                    if (h.dict.size() / 8 >= 0xFFFFFFFFu - R1CS_KIND_DICT) return snprintf(msg, sizeof msg, "entry %zu: too many distinct coefficients", i), bad(-2);
                    it = index.emplace(key, (uint32_t)(h.dict.size() / 8)).first;
                    h.dict.insert(h.dict.end(), key.begin(), key.end());
                }
                k = R1CS_KIND_DICT + it->second;
            }
        }
        kind[i] = k;
        info.plus_one += k == R1CS_KIND_PLUS;
        info.minus_one += k == R1CS_KIND_MINUS;
    }
    info.distinct_values = h.dict.size() / 8;

    // items, in (matrix, row) order
    const uint32_t n = 1u << log_n;
    std::vector<uint32_t> item_src;  // the sorted position of each item's first entry
    uint64_t n_partials = 0;
    for (uint32_t m = 0; m < 3; m++) {
        if (info.entries[m]) {
            for (uint32_t row = 0; row < num_rows; row++) {
                const size_t k = (size_t)m * num_rows + row;
                const uint32_t off = start[k], cnt = start[k + 1] - start[k];
                if (cnt <= R1CS_ITEM_LEN) {
                    if (layout) h.items.push_back(make_uint2(m * n + row, cnt)), item_src.push_back(off);
                    info.work_items++;
                    if (cnt > info.max_item_len) info.max_item_len = cnt;
                    continue;
                }
                const uint32_t pieces = (cnt + R1CS_ITEM_LEN - 1) / R1CS_ITEM_LEN;
                if (n_partials + pieces > 0xFFFFFFFFull) return snprintf(msg, sizeof msg, "too many partial sums"), bad(-2);
                if (layout) {
                    h.folds.push_back(make_uint4(m * n + row, (uint32_t)n_partials, pieces, 0));
                    for (uint32_t p = 0; p < pieces; p++) {
                        const uint32_t len = p + 1 < pieces ? R1CS_ITEM_LEN : cnt - p * R1CS_ITEM_LEN;
                        h.items.push_back(make_uint2((uint32_t)n_partials + p, len | R1CS_ITEM_PARTIAL));
                        item_src.push_back(off + p * R1CS_ITEM_LEN);
                    }
                }
                info.work_items += pieces;
                info.fold_rows++;
                info.max_item_len = R1CS_ITEM_LEN;
                n_partials += pieces;
            }
        }
        if (info.work_items > 0xFFFFFFFFull - R1CS_GROUP) return snprintf(msg, sizeof msg, "too many work items"), bad(-2);
        if (m == 1) h.items01 = (uint32_t)info.work_items, h.folds01 = (uint32_t)info.fold_rows;
    }
    info.partial_sums = n_partials;

    // layout: a group is as wide as its longest item
    const uint64_t groups = (info.work_items + R1CS_GROUP - 1) / R1CS_GROUP;
    uint64_t steps = 0;
    if (layout) {
        h.group_base.resize(groups);
        for (uint64_t g = 0; g < groups; g++) {
            uint32_t width = 0;
            for (uint64_t i = g * R1CS_GROUP; i < (g + 1) * R1CS_GROUP && i < info.work_items; i++) {
                const uint32_t len = h.items[i].y & ~R1CS_ITEM_PARTIAL;
                if (len > width) width = len;
            }
            if (steps > 0xFFFFFFFFull) return snprintf(msg, sizeof msg, "the entry array exceeds 2^38 slots"), bad(-2);
            h.group_base[g] = (uint32_t)steps;
            steps += width;
        }
        std::vector<uint32_t> order(n_coefs);  // the counting sort's scatter: stable
        {
            std::vector<uint32_t> cur(start.begin(), start.end() - 1);
            for (size_t i = 0; i < n_coefs; i++) order[cur[(size_t)coefs[i].matrix * num_rows + coefs[i].row]++] = (uint32_t)i;
        }
        h.entries.assign((size_t)steps * R1CS_GROUP, make_uint2(0, 0));
        for (uint64_t i = 0; i < info.work_items; i++) {
            const uint32_t len = h.items[i].y & ~R1CS_ITEM_PARTIAL;
            uint2* e = h.entries.data() + ((size_t)h.group_base[i / R1CS_GROUP] * R1CS_GROUP + i % R1CS_GROUP);
            for (uint32_t j = 0; j < len; j++) {
                const uint32_t src = order[item_src[i] + j];
                e[(size_t)j * R1CS_GROUP] = make_uint2(coefs[src].col, kind[src]);
            }
        }
        info.device_bytes = h.items.size() * 8 + h.group_base.size() * 4 + h.entries.size() * 8 + h.dict.size() * 4 + h.folds.size() * 16 + n_partials * 32;
    } else {
        // the same figure without building the arrays: the widths follow from the item lengths alone
        uint64_t i = 0;
        uint32_t width = 0;
        auto put = [&](uint32_t len) {
            if (len > width) width = len;
            if (++i % R1CS_GROUP == 0) steps += width, width = 0;
        };
        for (uint32_t m = 0; m < 3; m++) {
            if (!info.entries[m]) continue;
            for (uint32_t row = 0; row < num_rows; row++) {
                const size_t k = (size_t)m * num_rows + row;
                uint32_t cnt = start[k + 1] - start[k];
                for (; cnt > R1CS_ITEM_LEN; cnt -= R1CS_ITEM_LEN) put(R1CS_ITEM_LEN);
                put(cnt);
            }
        }
        steps += width;
        info.device_bytes = info.work_items * 8 + groups * 4 + steps * R1CS_GROUP * 8 + h.dict.size() * 4 + info.fold_rows * 16 + n_partials * 32;
    }
    return 0;
}

#if defined(__HIPCC__) && !defined(NTT_NO_KERNELS)
__global__ void __launch_bounds__(256) k_r1cs_items(const R1csView v, uint32_t n_items, const uint32_t* wit, const fr post, uint32_t* out, uint32_t* partials) {
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item < n_items) r1cs_item(v, item, wit, post, out, partials);
}
__global__ void __launch_bounds__(R1CS_GROUP) k_r1cs_fold(const R1csView v, const uint32_t* partials, const fr post, uint32_t* out) {
    __shared__ uint32_t sums[9 * R1CS_GROUP];
    const uint4 f = v.folds[blockIdx.x];
    ntt_lds_put(sums, threadIdx.x, r1cs_fold_lane(partials, f.y, f.z, threadIdx.x));
    __syncthreads();
    if (threadIdx.x == 0) r1cs_fold_finish(sums, post, out + (size_t)f.x * 8);
}
#endif

}  // namespace r1csk
