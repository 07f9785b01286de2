// Device neighbour list (cell list) -> CSR edge list sorted by (i, j, S), gfx950.
//
// Replaces the graph-building step in front of the hot path: ASE
// primitive_neighbor_list('ijDS', pbc, cell, pos, cutoff, self_interaction=True)
// followed by the removal of the i == j, S == 0 pair in the reference
// (sevenn/train/dataload.py:31-68, :113-125), and the host loops over LAMMPS'
// full neighbour list in pair_e3gnn.cpp:155-182.
//
// Edge (i, j, S): r_ij = (pos[j] + S cell) - pos[i], |r_ij|^2 < rc^2, S integer,
// excluding i == j with S == 0.  The inclusion test is evaluated in f64 in
// exactly this operation order with contraction off, the same arithmetic as the
// host list (neighbor.py), so both give the same edges bit for bit.  Binning
// only accelerates the search: atoms are wrapped into the cell, binned with bin
// widths >= rc, and every centre scans the (2R+1)^3 bin images around its bin
// (distinct (bin, image) pairs, so every periodic image is visited once).
//
// Pass 1 counts each centre's edges (one wave per centre, ballot), a scan gives
// the CSR offsets, pass 2 recomputes the hits into LDS, sorts the centre's keys
// (j, Sx, Sy, Sz) with a bitonic network and writes them: deterministic.
//
// The binning (nl_bin) and the search (nl_search) exist once.  The single and
// the rank build pass their one geometry as a kernel argument (k_nl_*); the
// batched form (k_nlb_*) runs the same bodies over many structures
// concatenated, each with its own geometry and bins (see "batch" below).
#include "neighbor.h"

#pragma clang fp contract(off)

namespace e3gnn {
namespace {

// err is int[1] (single and rank build) or int[4] (BATCH: the flags and, for
// bit 1, 2, 4, 1 + the largest offending structure index in err[1], [2], [3])
template <bool BATCH>
__device__ __forceinline__ void nl_flag(int* __restrict__ err, int bit, int st) {
  atomicOr(err, bit);
  if constexpr (BATCH) atomicMax(err + (bit == 1 ? 1 : bit == 2 ? 2 : 3), st + 1);
}

// ---------------------------------------------------------------- binning
// atom a of structure st (geometry G, first bin bin_base): f0 = floor of its
// fractional coordinates, bin = the bin of the wrapped remainder
template <bool BATCH>
__device__ __forceinline__ void nl_bin(int a, const double* __restrict__ pos, const NlGeom& G,
                                       int bin_base, int st, int* __restrict__ f0,
                                       int* __restrict__ bin, int* __restrict__ bin_count,
                                       int* __restrict__ err) {
  const double p0 = pos[3 * a] - G.origin[0], p1 = pos[3 * a + 1] - G.origin[1],
               p2 = pos[3 * a + 2] - G.origin[2];
  int b[3], fl3[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double f = ((p0 * G.inv[k]) + (p1 * G.inv[3 + k])) + (p2 * G.inv[6 + k]);
    const double fl = floor(f);
    const double fw = f - fl;
    int bk = (int)(fw * G.nb[k]);
    bk = bk < 0 ? 0 : (bk >= G.nb[k] ? G.nb[k] - 1 : bk);
    b[k] = bk;
    if (!(fl > -1e9 && fl < 1e9)) nl_flag<BATCH>(err, 1, st);  // non-finite or absurd position
    fl3[k] = (int)fl;
    f0[3 * a + k] = fl3[k];
  }
  if (!G.periodic && (fl3[0] | fl3[1] | fl3[2])) nl_flag<BATCH>(err, 1, st);
  const int id = bin_base + ((b[0] * G.nb[1] + b[1]) * G.nb[2] + b[2]);
  bin[a] = id;
  atomicAdd(&bin_count[id], 1);
}
__global__ void k_nl_bin(int n, const double* __restrict__ pos, NlGeom G, int* __restrict__ f0,
                         int* __restrict__ bin, int* __restrict__ bin_count, int* __restrict__ err) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a < n) nl_bin<false>(a, pos, G, 0, 0, f0, bin, bin_count, err);
}
__global__ void k_nlb_bin(int n, const double* __restrict__ pos,
                          const NlGeomB* __restrict__ geoms, const int* __restrict__ batch,
                          int* __restrict__ f0, int* __restrict__ bin,
                          int* __restrict__ bin_count, int* __restrict__ err) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  const int st = batch[a];
  nl_bin<true>(a, pos, geoms[st].G, geoms[st].bin_base, st, f0, bin, bin_count, err);
}

__global__ void k_nl_place(int n, const int* __restrict__ bin, const int* __restrict__ bin_start,
                           int* __restrict__ cursor, int* __restrict__ bin_atoms) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  const int id = bin[a];
  bin_atoms[bin_start[id] + atomicAdd(&cursor[id], 1)] = a;
}

// ---------------------------------------------------------------- search
// key = j << 33 | (Sx + 2^10) << 22 | (Sy + 2^10) << 11 | (Sz + 2^10): ascending
// keys are ascending (j, Sx, Sy, Sz)
constexpr int SB = 10;
__device__ __forceinline__ unsigned long long nl_key(int j, int sx, int sy, int sz) {
  return ((unsigned long long)j << 33) | ((unsigned long long)(sx + (1 << SB)) << 22) |
         ((unsigned long long)(sy + (1 << SB)) << 11) | (unsigned long long)(sz + (1 << SB));
}

struct Hit {
  double d[3];
};
// r_ij for (i, j, S): (pos_j + S cell) - pos_i, the host list's operation order
__device__ __forceinline__ Hit nl_vec(const double* __restrict__ pos, const NlGeom& G, int i,
                                      int j, int sx, int sy, int sz) {
  Hit h;
  const double s0 = sx, s1 = sy, s2 = sz;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const double sc = ((s0 * G.cell[d]) + (s1 * G.cell[3 + d])) + (s2 * G.cell[6 + d]);
    h.d[d] = (pos[3 * j + d] + sc) - pos[3 * i + d];
  }
  return h;
}

// one wave per centre; FILL = false: count, true: collect, sort, write.
// RANK = true is the rank-graph form (NlRank): the n centres are a list of atom
// ids, the count pass also flags boundary centres and ghost atoms, and the fill
// pass writes local rows (the centre's position in the list, lid[j]) while the
// keys still sort by the global (j, S).
// BATCH = true is the batched form: centre ci belongs to structure st, whose
// geometry is G and whose bins start at bin_base; rows, bins and keys are those
// of the concatenated batch, so a structure's edges come out in the single
// build's order with its first row added to i and j.
// K: the wave's NL_MAXD sort keys in LDS.
template <bool FILL, bool RANK, bool BATCH>
__device__ __forceinline__ void nl_search(
    int ci, const double* __restrict__ pos, const NlGeom& G, int bin_base, int st,
    unsigned long long* __restrict__ K, const int* __restrict__ f0,
    const int* __restrict__ bin, const int* __restrict__ bin_start,
    const int* __restrict__ bin_atoms, int* __restrict__ deg, const int* __restrict__ row_ptr,
    int* __restrict__ center, int* __restrict__ nbr, int* __restrict__ shift,
    float* __restrict__ vec, int* __restrict__ err, const NlRank& rk) {
  const int lane = threadIdx.x & 63;
  const int i = RANK ? __builtin_amdgcn_readfirstlane(rk.centers[ci]) : ci;
  const int bi = bin[i] - bin_base;
  const int b[3] = {bi / (G.nb[1] * G.nb[2]), (bi / G.nb[2]) % G.nb[1], bi % G.nb[2]};
  const int fi[3] = {f0[3 * i], f0[3 * i + 1], f0[3 * i + 2]};
  const double rc2 = G.rc2;
  int count = 0;  // uniform
  bool boundary = false;  // uniform (RANK count pass)
  for (int ox = -G.R[0]; ox <= G.R[0]; ++ox)
    for (int oy = -G.R[1]; oy <= G.R[1]; ++oy)
      for (int oz = -G.R[2]; oz <= G.R[2]; ++oz) {
        const int o[3] = {ox, oy, oz};
        int c[3], sh[3];
        bool skip = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const int v = b[k] + o[k];
          if (G.periodic) {
            sh[k] = v >= 0 ? v / G.nb[k] : -((-v + G.nb[k] - 1) / G.nb[k]);
            c[k] = v - sh[k] * G.nb[k];
          } else {
            sh[k] = 0;
            c[k] = v;
            skip |= v < 0 || v >= G.nb[k];
          }
        }
        if (skip) continue;
        const int id = bin_base + ((c[0] * G.nb[1] + c[1]) * G.nb[2] + c[2]);
        const int s = bin_start[id], e = bin_start[id + 1];
        for (int t0 = s; t0 < e; t0 += 64) {
          const int t = t0 + lane;
          bool hit = false;
          int j = 0, S[3] = {0, 0, 0};
          if (t < e) {
            j = bin_atoms[t];
#pragma unroll
            for (int k = 0; k < 3; ++k) S[k] = sh[k] + fi[k] - f0[3 * j + k];
            const Hit h = nl_vec(pos, G, i, j, S[0], S[1], S[2]);
            const double r2 = ((h.d[0] * h.d[0]) + (h.d[1] * h.d[1])) + (h.d[2] * h.d[2]);
            hit = r2 < rc2 && !(j == i && S[0] == 0 && S[1] == 0 && S[2] == 0);
          }
          const unsigned long long m = __ballot(hit);
          if constexpr (RANK && !FILL) {
            // same-value stores: the flags do not depend on the order of arrival
            const bool foreign = hit && rk.owner[j] != rk.rank;
            if (foreign) rk.ghost_flag[j] = 1;
            boundary |= __ballot(foreign) != 0;
          }
          if (FILL && hit) {
            const int slot = count + __popcll(m & ((1ull << lane) - 1));
            const int lim = 1 << SB;
            if (S[0] < -lim || S[0] >= lim || S[1] < -lim || S[1] >= lim || S[2] < -lim ||
                S[2] >= lim) {
              // the call fails, but the sort and the write-out below still decode
              // this slot: give it a key they can index with (this j, no shift)
              nl_flag<BATCH>(err, 2, st);
              S[0] = S[1] = S[2] = 0;
            }
            if (slot < NL_MAXD) K[slot] = nl_key(j, S[0], S[1], S[2]);
          }
          count += __popcll(m);
        }
      }
  if constexpr (!FILL) {
    if (lane == 0) {
      deg[ci] = count;
      if constexpr (RANK) rk.boundary_flag[ci] = boundary ? 1 : 0;
      if (count > NL_MAXD) nl_flag<BATCH>(err, 4, st);
    }
    return;
  } else {
    if (count > NL_MAXD) return;  // reported by the count pass
    // bitonic sort of K[0..P) (P = next power of two; padding = max key)
    int P = 1;
    while (P < count) P <<= 1;
    for (int t = count + lane; t < P; t += 64) K[t] = ~0ull;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (int k = 2; k <= P; k <<= 1)
      for (int jj = k >> 1; jj > 0; jj >>= 1) {
        for (int t = lane; t < P; t += 64) {
          const int u = t ^ jj;
          if (u > t) {
            const unsigned long long a = K[t], c = K[u];
            const bool up = (t & k) == 0;
            if ((a > c) == up) {
              K[t] = c;
              K[u] = a;
            }
          }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    const int base = row_ptr[ci];
    for (int t = lane; t < count; t += 64) {
      const unsigned long long key = K[t];
      const int j = (int)(key >> 33);
      const int sx = (int)((key >> 22) & 0x7ff) - (1 << SB);
      const int sy = (int)((key >> 11) & 0x7ff) - (1 << SB);
      const int sz = (int)(key & 0x7ff) - (1 << SB);
      const Hit h = nl_vec(pos, G, i, j, sx, sy, sz);
      const int64_t q = (int64_t)base + t;
      center[q] = ci;
      nbr[q] = RANK ? rk.lid[j] : j;
      if (shift) {
        shift[3 * q] = sx;
        shift[3 * q + 1] = sy;
        shift[3 * q + 2] = sz;
      }
      if (vec) {
        vec[3 * q] = (float)h.d[0];
        vec[3 * q + 1] = (float)h.d[1];
        vec[3 * q + 2] = (float)h.d[2];
      }
    }
  }
}
// The entry points own the sort keys (four waves, four centres per workgroup)
// and name the wave's centre.  Single and rank build: the geometry by value.
template <bool FILL, bool RANK>
__global__ __launch_bounds__(256) void k_nl_search(
    int n, const double* __restrict__ pos, NlGeom G, const int* __restrict__ f0,
    const int* __restrict__ bin, const int* __restrict__ bin_start,
    const int* __restrict__ bin_atoms, int* __restrict__ deg, const int* __restrict__ row_ptr,
    int* __restrict__ center, int* __restrict__ nbr, int* __restrict__ shift,
    float* __restrict__ vec, int* __restrict__ err, NlRank rk) {
  __shared__ unsigned long long keys[4][NL_MAXD];
  const int wid = threadIdx.x >> 6;
  const int ci = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wid);
  if (ci >= n) return;
  nl_search<FILL, RANK, false>(ci, pos, G, 0, 0, keys[wid], f0, bin, bin_start, bin_atoms, deg,
                               row_ptr, center, nbr, shift, vec, err, rk);
}
// Batch: the geometry of the centre's structure, a wave-uniform address.
template <bool FILL>
__global__ __launch_bounds__(256) void k_nlb_search(
    int n, const double* __restrict__ pos, const NlGeomB* __restrict__ geoms,
    const int* __restrict__ batch, const int* __restrict__ f0, const int* __restrict__ bin,
    const int* __restrict__ bin_start, const int* __restrict__ bin_atoms, int* __restrict__ deg,
    const int* __restrict__ row_ptr, int* __restrict__ center, int* __restrict__ nbr,
    int* __restrict__ shift, float* __restrict__ vec, int* __restrict__ err) {
  __shared__ unsigned long long keys[4][NL_MAXD];
  const int wid = threadIdx.x >> 6;
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wid);
  if (i >= n) return;
  const int st = __builtin_amdgcn_readfirstlane(batch[i]);
  nl_search<FILL, false, true>(i, pos, geoms[st].G, geoms[st].bin_base, st, keys[wid], f0, bin,
                               bin_start, bin_atoms, deg, row_ptr, center, nbr, shift, vec, err,
                               NlRank{});
}

// ---------------------------------------------------------------- rank graph
// Row order of one rank of a spatial decomposition (parallel.py RankGraph):
// owned atoms interior-first then boundary, each by id; ghosts by (owner, id).
// Every position below comes from a scan or a ballot, never from the order in
// which threads arrive, so the outputs are bitwise reproducible.

// mine[a] = 1 for the rank's atoms; owner values outside [0, world) -> err bit 8
__global__ void k_rk_mark(int n, const int* __restrict__ owner, int rank, int world,
                          int* __restrict__ mine, int* __restrict__ err) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  const int o = owner[a];
  if (o < 0 || o >= world) atomicOr(err, 8);
  mine[a] = o == rank ? 1 : 0;
}

// out[pos[a]] = a for every flagged a (pos = exclusive scan of flag): ascending ids
__global__ void k_rk_compact(int n, const int* __restrict__ flag, const int* __restrict__ pos,
                             int* __restrict__ out) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n) return;
  if (flag[a]) out[pos[a]] = a;
}

// centre c of the id-ordered list -> its local row (bpos = exclusive scan of the
// boundary flags, bpos[nc] = number of boundary centres); owned, the degrees in
// row order and lid of the owned atoms
__global__ void k_rk_rows(int nc, const int* __restrict__ centers, const int* __restrict__ bflag,
                          const int* __restrict__ bpos, const int* __restrict__ deg,
                          int* __restrict__ owned, int* __restrict__ deg_row,
                          int* __restrict__ lid) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int n_interior = nc - bpos[nc];
  const int r = bflag[c] ? n_interior + bpos[c] : c - bpos[c];
  const int a = centers[c];
  owned[r] = a;
  deg_row[r] = deg[c];
  lid[a] = r;
}

// Stable counting sort of the id-ordered ghost list by owner, blocks of 256
// ghosts.  A ghost's place inside its block among those of the same owner:
// its lane's rank in the wave's ballot of that owner plus the counts of the
// block's earlier waves.  SCATTER = false writes the per-block histogram
// hist[o * nblk + b]; after its exclusive scan (off), SCATTER = true places
// the ghosts and completes lid.
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_rk_ghost_sort(
    int ng, int world, int nblk, const int* __restrict__ gid, const int* __restrict__ owner,
    int* __restrict__ hist, const int* __restrict__ off, int n_local, int* __restrict__ ghosts,
    int* __restrict__ lid) {
  __shared__ int cnt[4][NL_MAX_WORLD];
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int t = threadIdx.x; t < 4 * NL_MAX_WORLD; t += 256) (&cnt[0][0])[t] = 0;
  __syncthreads();
  const int g = blockIdx.x * 256 + threadIdx.x;
  const bool live = g < ng;
  const int a = live ? gid[g] : 0;
  const int o = live ? owner[a] : -1;
  int in_wave = 0;
  bool todo = live;
  while (__ballot(todo)) {  // one round per distinct owner in the wave
    const unsigned long long act = __ballot(todo);
    const int lead = __ffsll((long long)act) - 1;
    const int v = __shfl(o, lead);
    const unsigned long long m = __ballot(todo && o == v);
    if (todo && o == v) {
      in_wave = __popcll(m & ((1ull << lane) - 1));
      if (lane == lead) cnt[wid][v] = __popcll(m);
      todo = false;
    }
  }
  __syncthreads();
  if constexpr (!SCATTER) {
    if ((int)threadIdx.x < world)
      hist[threadIdx.x * nblk + blockIdx.x] = ((cnt[0][threadIdx.x] + cnt[1][threadIdx.x]) +
                                               cnt[2][threadIdx.x]) + cnt[3][threadIdx.x];
  } else if (live) {
    int before = in_wave;
    for (int w = 0; w < wid; ++w) before += cnt[w][o];
    const int q = off[o * nblk + blockIdx.x] + before;
    ghosts[q] = a;
    lid[a] = n_local + q;
  }
}

// recv_counts[o] = ghosts of owner o, from the scanned histogram
__global__ void k_rk_recv(int world, int nblk, const int* __restrict__ off,
                          long long* __restrict__ recv_counts) {
  const int o = blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= world) return;
  recv_counts[o] = (long long)off[(o + 1) * nblk] - off[o * nblk];
}

// ---------------------------------------------------------------- batch
// B structures concatenated: the passes of the single build over all rows at
// once.  A thread (k_nlb_bin) or a wave (k_nlb_search) reads its structure's
// geometry from geoms[batch[row]]; bins are numbered through the whole batch
// (NlGeomB::bin_base), so the bin arrays, k_nl_place and both scans serve as
// they are, and a centre only ever meets atoms of its own structure.  The
// bodies are nl_bin and nl_search above; what is left here fills batch[] and
// the per-structure edge offsets.

__global__ void k_nlb_batch(const int* __restrict__ atom_ptr, int* __restrict__ batch) {
  const int s = blockIdx.x;
  for (int a = atom_ptr[s] + threadIdx.x; a < atom_ptr[s + 1]; a += blockDim.x) batch[a] = s;
}

__global__ void k_nlb_edge_ptr(int B, const int* __restrict__ atom_ptr,
                               const int* __restrict__ row_ptr, long long* __restrict__ edge_ptr) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s <= B) edge_ptr[s] = row_ptr[atom_ptr[s]];
}

}  // namespace

hipError_t launch_nl_bin(int n, const double* pos, const NlGeom& G, int* f0, int* bin,
                         int* bin_count, int* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_nl_bin, dim3((n + 255) / 256), dim3(256), 0, s, n, pos, G, f0, bin,
                     bin_count, err);
  return hipGetLastError();
}
hipError_t launch_nl_place(int n, const int* bin, const int* bin_start, int* cursor,
                           int* bin_atoms, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_nl_place, dim3((n + 255) / 256), dim3(256), 0, s, n, bin, bin_start,
                     cursor, bin_atoms);
  return hipGetLastError();
}
hipError_t launch_nl_search(bool fill, int n, const double* pos, const NlGeom& G, const int* f0,
                            const int* bin, const int* bin_start, const int* bin_atoms, int* deg,
                            const int* row_ptr, int* center, int* nbr, int* shift, float* vec,
                            int* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((n + 3) / 4), block(256);
  if (fill)
    hipLaunchKernelGGL((k_nl_search<true, false>), grid, block, 0, s, n, pos, G, f0, bin,
                       bin_start, bin_atoms, deg, row_ptr, center, nbr, shift, vec, err, NlRank{});
  else
    hipLaunchKernelGGL((k_nl_search<false, false>), grid, block, 0, s, n, pos, G, f0, bin,
                       bin_start, bin_atoms, deg, row_ptr, center, nbr, shift, vec, err, NlRank{});
  return hipGetLastError();
}
hipError_t launch_nl_rank_search(bool fill, int nc, const double* pos, const NlGeom& G,
                                 const int* f0, const int* bin, const int* bin_start,
                                 const int* bin_atoms, int* deg, const int* row_ptr, int* center,
                                 int* nbr, int* shift, float* vec, int* err, const NlRank& rk,
                                 hipStream_t s) {
  if (nc <= 0) return hipSuccess;
  const dim3 grid((nc + 3) / 4), block(256);
  if (fill)
    hipLaunchKernelGGL((k_nl_search<true, true>), grid, block, 0, s, nc, pos, G, f0, bin,
                       bin_start, bin_atoms, deg, row_ptr, center, nbr, shift, vec, err, rk);
  else
    hipLaunchKernelGGL((k_nl_search<false, true>), grid, block, 0, s, nc, pos, G, f0, bin,
                       bin_start, bin_atoms, deg, row_ptr, center, nbr, shift, vec, err, rk);
  return hipGetLastError();
}
hipError_t launch_rk_mark(int n, const int* owner, int rank, int world, int* mine, int* err,
                          hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rk_mark, dim3((n + 255) / 256), dim3(256), 0, s, n, owner, rank, world,
                     mine, err);
  return hipGetLastError();
}
hipError_t launch_rk_compact(int n, const int* flag, const int* pos, int* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rk_compact, dim3((n + 255) / 256), dim3(256), 0, s, n, flag, pos, out);
  return hipGetLastError();
}
hipError_t launch_rk_rows(int nc, const int* centers, const int* bflag, const int* bpos,
                          const int* deg, int* owned, int* deg_row, int* lid, hipStream_t s) {
  if (nc <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rk_rows, dim3((nc + 255) / 256), dim3(256), 0, s, nc, centers, bflag, bpos,
                     deg, owned, deg_row, lid);
  return hipGetLastError();
}
hipError_t launch_rk_ghost_sort(bool scatter, int ng, int world, int nblk, const int* gid,
                                const int* owner, int* hist, const int* off, int n_local,
                                int* ghosts, int* lid, hipStream_t s) {
  if (world < 1 || world > NL_MAX_WORLD || nblk < 1 || (int64_t)nblk * 256 < ng)
    return hipErrorInvalidValue;
  if (scatter)
    hipLaunchKernelGGL(k_rk_ghost_sort<true>, dim3(nblk), dim3(256), 0, s, ng, world, nblk, gid,
                       owner, hist, off, n_local, ghosts, lid);
  else
    hipLaunchKernelGGL(k_rk_ghost_sort<false>, dim3(nblk), dim3(256), 0, s, ng, world, nblk, gid,
                       owner, hist, off, n_local, ghosts, lid);
  return hipGetLastError();
}
hipError_t launch_rk_recv(int world, int nblk, const int* off, int64_t* recv_counts,
                          hipStream_t s) {
  hipLaunchKernelGGL(k_rk_recv, dim3((world + 63) / 64), dim3(64), 0, s, world, nblk, off,
                     (long long*)recv_counts);
  return hipGetLastError();
}

hipError_t launch_nlb_batch(int B, const int* atom_ptr, int* batch, hipStream_t s) {
  if (B <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_nlb_batch, dim3(B), dim3(256), 0, s, atom_ptr, batch);
  return hipGetLastError();
}
hipError_t launch_nlb_bin(int n, const double* pos, const NlGeomB* geoms, const int* batch, int* f0,
                          int* bin, int* bin_count, int* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_nlb_bin, dim3((n + 255) / 256), dim3(256), 0, s, n, pos, geoms, batch, f0,
                     bin, bin_count, err);
  return hipGetLastError();
}
hipError_t launch_nlb_search(bool fill, int n, const double* pos, const NlGeomB* geoms,
                             const int* batch, const int* f0, const int* bin,
                             const int* bin_start, const int* bin_atoms, int* deg,
                             const int* row_ptr, int* center, int* nbr, int* shift, float* vec,
                             int* err, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 grid((n + 3) / 4), block(256);
  if (fill)
    hipLaunchKernelGGL(k_nlb_search<true>, grid, block, 0, s, n, pos, geoms, batch, f0, bin,
                       bin_start, bin_atoms, deg, row_ptr, center, nbr, shift, vec, err);
  else
    hipLaunchKernelGGL(k_nlb_search<false>, grid, block, 0, s, n, pos, geoms, batch, f0, bin,
                       bin_start, bin_atoms, deg, row_ptr, center, nbr, shift, vec, err);
  return hipGetLastError();
}
hipError_t launch_nlb_edge_ptr(int B, const int* atom_ptr, const int* row_ptr, int64_t* edge_ptr,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_nlb_edge_ptr, dim3((B + 1 + 255) / 256), dim3(256), 0, s, B, atom_ptr,
                     row_ptr, (long long*)edge_ptr);
  return hipGetLastError();
}

}  // namespace e3gnn
