// sicp_voxel.hip -- at most one point per voxel of a lattice (include/simpleicp_hip_voxel.h; contract (V)).
// Two passes over the candidates.  k_voxel_insert reads each candidate's coordinates where the slot holds them, forms the voxel by
// the contract's formula, packs it into a 63-bit key relative to the lattice index of the slot's bounding box (21 bits per axis) and
// settles "lowest index per key" in an open-addressing hash table of {key, winner} word pairs: the key's slot is claimed by
// compare-and-swap, the winner by an atomic minimum -- so the table's final content is a function of the candidate SET, whatever
// order the lanes arrive in.  k_voxel_verdict then writes keep = (winner of my slot == me).  Nothing here loops without a bound.
#include "sicp_host.h"
#include "sicp_lanes.h"
#include "../../include/simpleicp_hip_voxel.h"

namespace sicp {
namespace {

constexpr int VX_BLOCK = 256;
constexpr int VX_MAX_BLOCKS = 4096;           // grid-stride beyond: one counter atomic per block at the end of the verdict pass
constexpr unsigned long long VX_EMPTY = ~0ull;    // no key has bit 63 set; no winner word reaches it (indices < 2^31)
constexpr int VX_BITS = 21;
constexpr double VX_EXTENT = 2097152.0;       // 2^21 cells per axis

struct VoxelLattice {
    double c, o[3], lo[3];                    // cell size, origin, lattice index of the bounding box's low corner per axis
};

// murmur3's 64-bit finaliser: every input bit reaches every output bit, so keys that differ in a few regular bit positions -- a
// point lattice whose spacing is a multiple of the cell -- spread over the table like random ones (a multiplicative hash maps them
// onto an arithmetic progression of slots)
__device__ __forceinline__ unsigned long long vx_hash(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// contract (V): floor((v - o) / c) with IEEE subtraction and division, relative to the box's lattice index; false: outside 2^21
__device__ __forceinline__ bool vx_axis(double v, double o, double c, double lo, unsigned long long *i)
{
    const double rel = __builtin_floor((v - o) / c) - lo;      // (both integers, |difference| small: exact)
    const bool in = rel >= 0.0 && rel < VX_EXTENT;
    *i = in ? (unsigned long long)rel : 0ull;                   // (converted only once it is known to fit)
    return in;
}

// cnt[1] |= 1: a coordinate outside the lattice the host sized; |= 2: no free slot within `cap` probes
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_insert(const double *__restrict__ x, const double *__restrict__ y,
                                                           const double *__restrict__ z, const int64_t *__restrict__ rows,
                                                           const uint8_t *__restrict__ mask, long m, VoxelLattice L,
                                                           unsigned long long *__restrict__ tab, unsigned long long cap_mask,
                                                           uint32_t *__restrict__ slot_of, unsigned *__restrict__ cnt)
{
    const long stride = (long)gridDim.x * VX_BLOCK;
    for (long i = (long)blockIdx.x * VX_BLOCK + threadIdx.x; i < m; i += stride) {
        if (mask && mask[i] == 0) continue;
        const long p = rows ? rows[i] : i;
        unsigned long long ix, iy, iz;
        const bool in_x = vx_axis(x[p], L.o[0], L.c, L.lo[0], &ix), in_y = vx_axis(y[p], L.o[1], L.c, L.lo[1], &iy),
                   in_z = vx_axis(z[p], L.o[2], L.c, L.lo[2], &iz);
        if (!(in_x && in_y && in_z)) { atomicOr(cnt + 1, 1u); slot_of[i] = 0; continue; }
        const unsigned long long key = (ix << (2 * VX_BITS)) | (iy << VX_BITS) | iz;
        const unsigned long long me = ((unsigned long long)p << 32) | (unsigned long long)i;     // lowest point, then lowest entry
        unsigned long long h = vx_hash(key) & cap_mask;
        bool placed = false;
        for (unsigned long long probe = 0; probe <= cap_mask; ++probe, h = (h + 1) & cap_mask) {
            unsigned long long *kw = tab + 2 * h;
            // a look before the atomic: a key word changes once (empty -> its key) and a winner word only falls, so a stale value
            // costs an atomic that was not needed and never skips one that was
            unsigned long long seen = __hip_atomic_load(kw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == VX_EMPTY) seen = atomicCAS(kw, VX_EMPTY, key);
            if (seen == VX_EMPTY || seen == key) {
                if (__hip_atomic_load(kw + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > me) atomicMin(kw + 1, me);
                slot_of[i] = (uint32_t)h;
                placed = true;
                break;
            }
        }
        if (!placed) { atomicOr(cnt + 1, 2u); slot_of[i] = 0; }
    }
}

// keep[i] = candidate i won its voxel (0 for a masked-out point); cnt[0] += the block's kept candidates
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_verdict(const int64_t *__restrict__ rows, const uint8_t *mask, long m,
                                                            const unsigned long long *__restrict__ tab,
                                                            const uint32_t *__restrict__ slot_of, uint8_t *keep,
                                                            unsigned *__restrict__ cnt)
{
    const long stride = (long)gridDim.x * VX_BLOCK;
    unsigned mine = 0;
    for (long i = (long)blockIdx.x * VX_BLOCK + threadIdx.x; i < m; i += stride) {
        bool k = false;
        if (!mask || mask[i] != 0) {                               // (keep may alias mask: byte i is read before it is written, by this lane alone)
            const unsigned long long p = (unsigned long long)(rows ? rows[i] : i);
            k = tab[2 * (unsigned long long)slot_of[i] + 1] == ((p << 32) | (unsigned long long)i);
        }
        keep[i] = k ? 1 : 0;
        mine += k ? 1u : 0u;
    }
    const unsigned t = block_sum_u32<VX_BLOCK / 64>(mine);
    if (threadIdx.x == 0 && t) atomicAdd(cnt, t);
}

// cnt[0] += the non-zero bytes of mask: how many candidates a masked call has (its table is sized by them, not by the cloud)
__global__ __launch_bounds__(VX_BLOCK) void k_voxel_count(const uint8_t *__restrict__ mask, long n,
                                                          unsigned long long *__restrict__ cnt)
{
    const long stride = (long)gridDim.x * VX_BLOCK;
    unsigned mine = 0;
    for (long i = (long)blockIdx.x * VX_BLOCK + threadIdx.x; i < n; i += stride) mine += mask[i] != 0 ? 1u : 0u;
    const unsigned t = block_sum_u32<VX_BLOCK / 64>(mine);
    if (threadIdx.x == 0 && t) atomicAdd(cnt, (unsigned long long)t);
}

}  // namespace
}  // namespace sicp

namespace {

// the checks both entries share, and the lattice over the slot's bounding box
int vx_lattice(sicp_ctx *c, int slot, double cell, const double *origin, VoxelLattice *L)
{
    if (!(cell > 0.0) || !std::isfinite(cell)) return fail(SICP_ERR_INVALID, "cell must be finite and > 0");
    L->c = cell;
    for (int a = 0; a < 3; ++a) {
        L->o[a] = origin ? origin[a] : 0.0;
        if (!std::isfinite(L->o[a])) return fail(SICP_ERR_INVALID, "origin must be finite");
    }
    CHK(check_whole_cloud(c, slot, "voxel selection", "the lowest index of a voxel may live on another rank"));
    const Cloud &cl = c->cloud[slot];
    for (int a = 0; a < 3; ++a) {
        // the contract's formula on the box's corners: floor and the two operations are monotone, so every point's index lies between
        const double lo = std::floor((cl.bb_lo[a] - L->o[a]) / cell), hi = std::floor((cl.bb_hi[a] - L->o[a]) / cell);
        const double extent = hi - lo + 1.0;
        if (!(extent <= VX_EXTENT))
            return fail(SICP_ERR_INVALID, "the voxel lattice spans %.0f cells along %c (cell %g, coordinates %g ... %g): at most 2097152 (2^21) "
                        "per axis -- choose a larger cell", extent, "xyz"[a], cell, cl.bb_lo[a], cl.bb_hi[a]);
        L->lo[a] = lo;
    }
    return SICP_OK;
}

// the masked form only counts its candidates: the table (and what is cleared of it) follows the mask's set bytes, not the cloud's size
int vx_count_mask(sicp_ctx *c, const uint8_t *mask, long n, unsigned long long *d_count, const int64_t **d_rows)
{
    const unsigned g = std::min(cdiv(n, VX_BLOCK), (unsigned)VX_MAX_BLOCKS);
    hipLaunchKernelGGL(k_voxel_count, dim3(g), dim3(VX_BLOCK), 0, c->stream, mask, n, d_count);
    *d_rows = nullptr;
    return SICP_OK;
}

// both passes over the candidates K, verdicts into d_keep (device), the count into *kept_out
int vx_run(sicp_ctx *c, int slot, const Candidates &K, const VoxelLattice &L, uint8_t *d_keep, int64_t *kept_out)
{
    const long m = K.positions;
    const Cloud &cl = c->cloud[slot];
    size_t cap = 1024;
    while (cap < 2 * (size_t)K.count) cap <<= 1;                    // load <= 0.5; fewer than 2^31 candidates, so at most 2^32 slots: their numbers fit 32 bits
    CHK(c->vx_tab.reserve(2 * cap));
    CHK(c->vx_slot.reserve((size_t)m));
    unsigned *cnt = (unsigned *)c->cand_small.p;                    // the first counter word as two 32-bit ones, written and read as such: [0] the kept [1] the error bits (cleared by take_candidates)
    HIPCHK(hipMemsetAsync(c->vx_tab.p, 0xff, 2 * cap * sizeof(unsigned long long), c->stream));
    const unsigned g = std::min(cdiv(m, VX_BLOCK), (unsigned)VX_MAX_BLOCKS);
    hipLaunchKernelGGL(k_voxel_insert, dim3(g), dim3(VX_BLOCK), 0, c->stream, cl.x(), cl.y(), cl.z(), K.d_rows, K.d_mask, m, L, c->vx_tab.p,
                       (unsigned long long)(cap - 1), c->vx_slot.p, cnt);
    hipLaunchKernelGGL(k_voxel_verdict, dim3(g), dim3(VX_BLOCK), 0, c->stream, K.d_rows, K.d_mask, m, c->vx_tab.p, c->vx_slot.p, d_keep,
                       cnt);
    HIPCHK(hipGetLastError());
    CHK(counters_fetch(c));
    CHK(sync(c));
    unsigned h_cnt[2];
    std::memcpy(h_cnt, counters_host(c), sizeof h_cnt);
    if (h_cnt[1] & 1u) return fail(SICP_ERR_INVALID, "a point lies outside the voxel lattice of the slot's bounding box (internal error)");
    if (h_cnt[1] & 2u) return fail(SICP_ERR_INVALID, "the voxel hash table is full (internal error)");
    *kept_out = (int64_t)h_cnt[0];
    return SICP_OK;
}

}  // namespace

SICP_EXPORT int sicp_voxel_version(void) { return SICP_VOXEL_VERSION; }

SICP_EXPORT int sicp_voxel_select(sicp_ctx *c, int slot, const int64_t *rows, int64_t m, double cell, const double *origin,
                                  uint8_t *keep_out, int64_t *kept_out)
{
    CHK(check_slot(c, slot, true));
    if (!keep_out || !kept_out) return fail(SICP_ERR_INVALID, "null argument");
    VoxelLattice L;
    CHK(vx_lattice(c, slot, cell, origin, &L));
    CHK(check_candidate_rows(rows, m, c->cloud[slot].n));
    HIPCHK(hipSetDevice(c->device));
    return op_run(c, [&]() -> int {
        Candidates K;
        CHK(take_candidates(c, slot, rows, m, nullptr, nullptr, &K));
        uint8_t *d_keep;
        CHK(stage_out(c, keep_out, (size_t)K.positions, c->cand_keep, &d_keep));
        CHK(vx_run(c, slot, K, L, d_keep, kept_out));
        if (d_keep == keep_out) return SICP_OK;
        CHK(stage_leave(c, keep_out, (size_t)K.positions, d_keep));
        return sync(c);
    });
}

SICP_EXPORT int sicp_voxel_select_masked(sicp_ctx *c, int slot, const uint8_t *mask, int64_t n, double cell, const double *origin,
                                         uint8_t *keep_out, int64_t *kept_out)
{
    CHK(check_slot(c, slot, true));
    if (!mask || !keep_out || !kept_out) return fail(SICP_ERR_INVALID, "null argument");
    VoxelLattice L;
    CHK(vx_lattice(c, slot, cell, origin, &L));
    if (n != c->cloud[slot].n) return fail(SICP_ERR_INVALID, "n must be the slot's size (%lld points)", (long long)c->cloud[slot].n);
    HIPCHK(hipSetDevice(c->device));
    CHK(check_device_ptr(c, keep_out, "keep_out"));
    return op_run(c, [&]() -> int {
        Candidates K;
        CHK(take_candidates(c, slot, nullptr, 0, mask, vx_count_mask, &K));
        if (K.count == 0) {
            HIPCHK(hipMemsetAsync(keep_out, 0, (size_t)n, c->stream));
            *kept_out = 0;
            return sync(c);
        }
        return vx_run(c, slot, K, L, keep_out, kept_out);
    });
}
