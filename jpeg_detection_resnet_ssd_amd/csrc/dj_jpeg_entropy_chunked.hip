// Huffman entropy decoding of JPEG files WITHOUT restart intervals (and of files with them, several short segments each) to
// their raw int16 coefficient planes, by chunks -- bit for bit what data/entropy_decode.py:chunked_decode_host states, which
// equals entropy_decode_host.  The scheme (chunks, positions, states, ownership of a symbol, the synchronisation's fixed
// point, the three output passes) is in that module's comment and is not repeated here.
//
// Five launches on one stream:
//   layout  one workgroup: the exclusive prefix sum over the files of their block counts -> where each file's DC
//           differences start in the scratch;
//   zero    one workgroup per file: its planes, 16 bytes a lane;
//   sync    ONE WORKGROUP PER SEGMENT, lanes stride over its chunks: every chunk decodes from its guess, then rounds of
//           "take the predecessor's exit, decode again if it differs from the entry last used" separated by
//           __syncthreads(), until the LDS flag says a round changed nothing (a `for` bounded by the chunk count; every
//           lane reaches every barrier, the break is on a value all lanes read); then the prefix sum of the chunks'
//           completed blocks, status 0 and "no failing block" for the segment;
//   final   one lane per chunk over the whole grid: decodes from the chunk's true entry, writes DC differences by block
//           index and AC coefficients -- a block that starts and ends in the chunk through the lane's LDS rows and eight
//           16-byte stores as in dj_jpeg_entropy_kernel, a block that straddles chunks element by element into the zeroed
//           planes -- and, for the one chunk of a segment that meets an error before the segment's last block, the status
//           and the failing block's index;
//   dc      one workgroup per segment: per component a workgroup-wide scan of the differences in scan order (int32
//           wrap-around), position 0 of every stored block in front of the failing one; the failing block is cleared.
//
// Scratch (dj_jpeg_entropy_chunked_scratch_bytes): [chunk records, 32 bytes each | first block of each file, 8 bytes |
// failing block of each segment, 4 bytes | DC differences, 2 bytes a block], each part at a multiple of 16 bytes.
//
// Safety: the host checks the host copies (dj_je_check_records, the chunk counts, the scratch); the kernels clamp what they
// read from the device copies again -- file and table indexes, byte ranges, chunk counts and first chunks, entry states
// (position into the segment's range, u, k, status), block counts and indexes -- and bound every store by the part's
// size, the plane's capacity and out_bytes.  Every loop has a bound the host fixed: chunks per segment, symbols per chunk
// (8 chunk_bytes + 8: a symbol consumes at least one bit), 25 steps of the binary search.  Plain C++ integer code.
#include "dj_jpeg_entropy_common.h"

#define DJ_JEC_SYNC_LANES 256
#define DJ_JEC_MAX_CHUNKS 65536

struct DjJecChunk {      // 32 bytes
  long entry_pos, exit_pos;
  int entry_state, exit_state;      // u | k << 8 | status << 16
  int blocks, first_block;
};

struct DjJecParams {
  const unsigned char* bytes;
  long n_bytes;
  const dj_jpeg_entropy_desc* desc;
  int n_files;
  const dj_jpeg_entropy_seg* seg;
  int n_segments;
  const unsigned char* tables;
  int n_tables;
  unsigned char* out;
  long out_bytes;
  int* status;
  int* rounds;
  DjJecChunk* chunks;
  long* file_first;      // first block of each file among the DC differences
  int* failing;          // per segment: the block it failed in, or its block count
  short* diffs;
  long total_chunks, total_blocks;
  int chunk_bytes;
  int max_mcus, max_chunks;      // the largest of the host's records
};

struct DjJecState {
  long pos;
  int u, k, status;
};

__device__ __forceinline__ int dj_jec_pack(const DjJecState& s) { return s.u | (s.k << 8) | (s.status << 16); }

// What a segment's lanes need of its records, clamped
struct DjJecSegment {
  long begin, end;
  int file, first_mcu, n_mcus, n_chunks;
  long chunk_first, diff_first;
  int ncomp, bpm, total;      // blocks per MCU, blocks of the segment
  int nb[3], hs[3], vs[3];    // blocks per MCU of each component, across, down
  const unsigned char *dc[3], *ac[3];
  int mcus_x;
};

__device__ __forceinline__ void dj_jec_segment(const DjJecParams& p, int s, DjJecSegment& g) {
  const dj_jpeg_entropy_seg* sg = p.seg + s;
  g.file = dj_je_clamp(sg->file, 0, p.n_files - 1);
  const dj_jpeg_entropy_desc* d = p.desc + g.file;
  g.end = min(max(sg->end, 0L), p.n_bytes);
  g.begin = min(max(sg->begin, 0L), g.end);
  g.n_mcus = dj_je_clamp(sg->n_mcus, 0, p.max_mcus);
  g.first_mcu = dj_je_clamp(sg->first_mcu, 0, 1 << 26);
  g.n_chunks = (int)min(max((g.end - g.begin + p.chunk_bytes - 1) / p.chunk_bytes, 1L), (long)p.max_chunks);
  g.chunk_first = min(max((long)sg->reserved, 0L), p.total_chunks - g.n_chunks);
  g.ncomp = d->n_components == 1 ? 1 : 3;
  g.mcus_x = max(d->mcus_x, 1);
  const int table_first = dj_je_clamp(d->table_first, 0, p.n_tables - 1);
  g.bpm = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    g.hs[c] = dj_je_clamp(d->h_blocks[c], 1, 4);
    g.vs[c] = dj_je_clamp(d->v_blocks[c], 1, 4);
    g.nb[c] = c < g.ncomp ? g.hs[c] * g.vs[c] : 0;
    g.bpm += g.nb[c];
    g.dc[c] = p.tables + (long)dj_je_clamp(table_first + dj_je_clamp(d->dc_table[c], 0, 3), 0, p.n_tables - 1) * DJ_JE_HUFF_BYTES;
    g.ac[c] = p.tables + (long)dj_je_clamp(table_first + dj_je_clamp(d->ac_table[c], 0, 3), 0, p.n_tables - 1) * DJ_JE_HUFF_BYTES;
  }
  g.total = g.n_mcus * g.bpm;      // <= max_mcus * 48
  g.diff_first = min(max(p.file_first[g.file], 0L), p.total_blocks) + (long)g.first_mcu * g.bpm;
}

__device__ __forceinline__ int dj_jec_component(const DjJecSegment& g, int u) { return u < g.nb[0] ? 0 : u < g.nb[0] + g.nb[1] ? 1 : 2; }

// Where block `index` of the segment (u its place in the MCU) lies in `out`: -> the byte offset, or -1 for a block that is
// not stored (MCU padding, or outside what the descriptor's capacity and out_bytes allow)
__device__ __forceinline__ long dj_jec_block_at(const DjJecParams& p, const DjJecSegment& g, int index, int u) {
  const dj_jpeg_entropy_desc* d = p.desc + g.file;
  const int c = dj_jec_component(g, u);
  const int j = u - (c == 0 ? 0 : c == 1 ? g.nb[0] : g.nb[0] + g.nb[1]);
  const int h = c == 0 ? g.hs[0] : c == 1 ? g.hs[1] : g.hs[2], v = c == 0 ? g.vs[0] : c == 1 ? g.vs[1] : g.vs[2];
  const int by = j / h, bx = j - by * h;
  const int mcu = g.first_mcu + index / g.bpm;
  const int my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
  const int bh = dj_je_clamp(d->blocks_h[c], 0, 8192), bw = dj_je_clamp(d->blocks_w[c], 0, 8192);
  const long plane = d->plane_offset[c], capacity = d->plane_capacity[c];
  const long row = (long)my * v + by, col = (long)mx * h + bx;
  const long at = plane + (row * bw + col) * 128;
  const bool store = row < bh && col < bw && plane >= 0 && (at & 15) == 0 && (row * bw + col + 1) * 64 <= capacity &&
                     at + 128 <= p.out_bytes;
  return store ? at : -1;
}

// Every symbol from `st` that starts before bit position `limit` of the segment.  FINAL: stops at the segment's last block,
// stores DC differences and AC coefficients (blk: the lane's LDS rows) and reports the block an error was met in.
template <bool FINAL>
__device__ __forceinline__ void dj_jec_decode(const DjJecParams& p, const DjJecSegment& g, DjJecState& st, long limit, int& blocks,
                                              int first_block, unsigned short* blk, const unsigned char* natural, int& failed) {
  blocks = 0;
  failed = -1;
  if (st.status != 0 || st.pos >= limit) return;
  DjJeBits b;
  b.bytes = p.bytes;
  b.end = g.end;
  b.p = min(max(st.pos >> 3, g.begin), g.end);
  b.acc = 0;
  b.nbits = 0;
  b.real = 0;
  b.stuffed = 0;
  const int bit = (int)(st.pos & 7);
  if (bit) {
    dj_je_fill(b);
    dj_je_skip(b, bit);
  }
  int u = st.u, k = st.k, status = 0;
  int c = dj_jec_component(g, u);
  const unsigned char *dc = c == 0 ? g.dc[0] : c == 1 ? g.dc[1] : g.dc[2], *ac = c == 0 ? g.ac[0] : c == 1 ? g.ac[1] : g.ac[2];
  bool whole = false;      // FINAL: the block under construction started in this chunk and lives in the LDS rows
  long at = FINAL ? dj_jec_block_at(p, g, first_block, u) : -1;
  long pos = st.pos;
  const int max_symbols = 8 * p.chunk_bytes + 8;
  for (int it = 0; it < max_symbols; ++it) {
    pos = dj_je_position(b);
    if (pos >= limit || (FINAL && first_block + blocks >= g.total)) break;
    int sym, l;
    bool complete = false;
    if (k == 0) {
      l = dj_je_symbol(b, dc, sym);
      if (l == 0) { status = 1; break; }
      dj_je_skip(b, l);
      if (b.real < 0) { status = 4; break; }
      if (sym > 11) { status = 1; break; }
      int diff = 0;
      if (sym) {
        dj_je_fill(b);
        const int v = (int)(b.acc >> (32 - sym));
        dj_je_skip(b, sym);
        if (b.real < 0) { status = 4; break; }
        diff = dj_je_extend(v, sym);
      }
      if (FINAL) {
        const long di = g.diff_first + first_block + blocks;
        if (di >= 0 && di < p.total_blocks) p.diffs[di] = (short)diff;
        whole = true;
      }
      k = 1;
    } else {
      l = dj_je_symbol(b, ac, sym);
      if (l == 0) { status = 2; break; }
      dj_je_skip(b, l);
      if (b.real < 0) { status = 4; break; }
      const int r = sym >> 4, s = sym & 15;
      int kk = k;
      if (s == 0) {
        if (r != 15) complete = true;
        kk += 16;
      } else {
        kk += r;
        if (kk > 63) { status = 3; break; }
        dj_je_fill(b);
        const int v = (int)(b.acc >> (32 - s));
        dj_je_skip(b, s);
        if (b.real < 0) { status = 4; break; }
        if (FINAL) {
          const int n = natural[kk];
          const unsigned short value = (unsigned short)dj_je_extend(v, s);
          if (whole) blk[(n >> 3) * (DJ_JE_LANES * 8) + (n & 7)] = value;
          else if (at >= 0) *reinterpret_cast<unsigned short*>(p.out + at + 2 * n) = value;
        }
        ++kk;
      }
      k = kk;
      if (k >= 64) complete = true;
    }
    if (complete) {
      if (FINAL && whole) {
        dj_je_row* rows = reinterpret_cast<dj_je_row*>(blk);
        const dj_je_row zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const dj_je_row value = rows[r * DJ_JE_LANES];
          rows[r * DJ_JE_LANES] = zero;
          if (at >= 0) *reinterpret_cast<dj_je_row*>(p.out + at + 16 * r) = value;
        }
        whole = false;
      }
      u = u + 1 >= g.bpm ? 0 : u + 1;
      k = 0;
      ++blocks;
      c = dj_jec_component(g, u);
      dc = c == 0 ? g.dc[0] : c == 1 ? g.dc[1] : g.dc[2];
      ac = c == 0 ? g.ac[0] : c == 1 ? g.ac[1] : g.ac[2];
      if (FINAL) at = dj_jec_block_at(p, g, first_block + blocks, u);
    }
    if (it + 1 == max_symbols) pos = dj_je_position(b);
  }
  if (FINAL && whole) {
    // the block goes on in the next chunk (its coefficients so far leave element by element) or failed (it stays zero)
    for (int n = 1; n < 64; ++n) {
      unsigned short* e = blk + (n >> 3) * (DJ_JE_LANES * 8) + (n & 7);
      const unsigned short value = *e;
      *e = 0;
      if (value && status == 0 && at >= 0) *reinterpret_cast<unsigned short*>(p.out + at + 2 * n) = value;
    }
  }
  if (status != 0) failed = first_block + blocks;
  st.pos = pos;      // of the failing symbol's start, or of the first symbol that is not this chunk's
  st.u = u;
  st.k = k;
  st.status = status;
}

__device__ __forceinline__ DjJecState dj_jec_unpack(const DjJecSegment& g, long pos, int packed) {
  DjJecState s;
  s.pos = min(max(pos, 8 * g.begin), 8 * g.end);
  s.u = dj_je_clamp(packed & 255, 0, g.bpm - 1);
  s.k = dj_je_clamp((packed >> 8) & 255, 0, 63);
  s.status = (packed >> 16) & 7;
  return s;
}

__device__ __forceinline__ long dj_jec_limit(const DjJecSegment& g, int chunk, int chunk_bytes) {
  return chunk + 1 < g.n_chunks ? 8 * (g.begin + (long)(chunk + 1) * chunk_bytes) : 8 * g.end;
}

// ---- layout: file_first[i] = the blocks of the files in front of file i -----------------------------------------------------
__global__ __launch_bounds__(DJ_JEC_SYNC_LANES) void dj_jec_layout_kernel(DjJecParams p) {
  __shared__ long part[DJ_JEC_SYNC_LANES];
  __shared__ long carry;
  const int lane = threadIdx.x;
  if (lane == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < p.n_files; base += DJ_JEC_SYNC_LANES) {      // uniform bounds: every lane reaches every barrier
    const int i = base + lane;
    long mine = 0;
    if (i < p.n_files) {
      const dj_jpeg_entropy_desc* d = p.desc + i;
      const int ncomp = d->n_components == 1 ? 1 : 3;
      int bpm = 0;
      for (int c = 0; c < ncomp; ++c) bpm += dj_je_clamp(d->h_blocks[c], 1, 4) * dj_je_clamp(d->v_blocks[c], 1, 4);
      mine = (long)dj_je_clamp(d->mcus_x, 1, 8192) * dj_je_clamp(d->mcus_y, 1, 8192) * bpm;
    }
    part[lane] = mine;
    __syncthreads();
    for (int step = 1; step < DJ_JEC_SYNC_LANES; step <<= 1) {
      const long add = lane >= step ? part[lane - step] : 0;
      __syncthreads();
      part[lane] += add;
      __syncthreads();
    }
    if (i < p.n_files) p.file_first[i] = min(carry + part[lane] - mine, p.total_blocks);
    __syncthreads();
    if (lane == 0) carry += part[DJ_JEC_SYNC_LANES - 1];
    __syncthreads();
  }
}

// ---- zero: every plane of every file ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(DJ_JEC_SYNC_LANES) void dj_jec_zero_kernel(DjJecParams p) {
  const dj_jpeg_entropy_desc* d = p.desc + blockIdx.x;
  const int ncomp = d->n_components == 1 ? 1 : 3;
  const dj_je_row zero = {0u, 0u, 0u, 0u};
  for (int c = 0; c < ncomp; ++c) {
    const long plane = d->plane_offset[c];
    const long blocks = (long)dj_je_clamp(d->blocks_h[c], 0, 8192) * dj_je_clamp(d->blocks_w[c], 0, 8192);
    const long rows = min(blocks * 8, max(d->plane_capacity[c], 0L) / 8);      // 16-byte rows
    if (plane < 0 || (plane & 15)) continue;
    for (long r = threadIdx.x; r < rows; r += DJ_JEC_SYNC_LANES)
      if (plane + 16 * r + 16 <= p.out_bytes) *reinterpret_cast<dj_je_row*>(p.out + plane + 16 * r) = zero;
  }
}

// ---- sync: the fixed point of the chunks' entry states, then their first blocks ------------------------------------------------
__global__ __launch_bounds__(DJ_JEC_SYNC_LANES) void dj_jec_sync_kernel(DjJecParams p) {
  __shared__ int changed;
  __shared__ int part[DJ_JEC_SYNC_LANES];
  __shared__ int carry;
  const int lane = threadIdx.x, s = blockIdx.x;
  DjJecSegment g;
  dj_jec_segment(p, s, g);      // the same for every lane: n_chunks is uniform
  DjJecChunk* chunks = p.chunks + g.chunk_first;
  if (lane == 0) {
    changed = 0;
    carry = 0;
  }
  int failed;
  // every chunk from its guess (chunk 0: the segment's start)
  for (int c = lane; c < g.n_chunks; c += DJ_JEC_SYNC_LANES) {
    long at = g.begin + (long)c * p.chunk_bytes;
    if (c > 0 && at < g.end && p.bytes[at] == 0x00 && p.bytes[at - 1] == 0xFF) ++at;
    DjJecState st;
    st.pos = 8 * min(at, g.end);
    st.u = st.k = st.status = 0;
    DjJecChunk rec;
    rec.entry_pos = st.pos;
    rec.entry_state = 0;
    dj_jec_decode<false>(p, g, st, dj_jec_limit(g, c, p.chunk_bytes), rec.blocks, 0, nullptr, nullptr, failed);
    rec.exit_pos = st.pos;
    rec.exit_state = dj_jec_pack(st);
    rec.first_block = 0;
    chunks[c] = rec;
  }
  __syncthreads();
  int rounds = 0;
  for (int round = 1; round < g.n_chunks; ++round) {      // chunk c is right after at most c rounds
    // take the predecessor's exit; a chunk whose entry changed is marked by first_block = -1
    for (int c = lane; c < g.n_chunks; c += DJ_JEC_SYNC_LANES)
      if (c > 0 && (chunks[c - 1].exit_pos != chunks[c].entry_pos || chunks[c - 1].exit_state != chunks[c].entry_state)) {
        chunks[c].first_block = -1;
        changed = 1;
      }
    __syncthreads();
    const bool go = changed != 0;
    __syncthreads();      // every lane has read the flag before it is cleared
    if (!go) break;       // the same value in every lane
    if (lane == 0) changed = 0;
    rounds = round;
    // entries first, behind a barrier: the exits they are copied from are this round's inputs
    for (int c = lane; c < g.n_chunks; c += DJ_JEC_SYNC_LANES)
      if (chunks[c].first_block < 0) {
        chunks[c].entry_pos = chunks[c - 1].exit_pos;
        chunks[c].entry_state = chunks[c - 1].exit_state;
      }
    __syncthreads();
    for (int c = lane; c < g.n_chunks; c += DJ_JEC_SYNC_LANES)
      if (chunks[c].first_block < 0) {
        DjJecState st = dj_jec_unpack(g, chunks[c].entry_pos, chunks[c].entry_state);
        int blocks;
        dj_jec_decode<false>(p, g, st, dj_jec_limit(g, c, p.chunk_bytes), blocks, 0, nullptr, nullptr, failed);
        chunks[c].exit_pos = st.pos;
        chunks[c].exit_state = dj_jec_pack(st);
        chunks[c].blocks = blocks;
        chunks[c].first_block = 0;
      }
    __syncthreads();
  }
  // exclusive prefix sum of the completed blocks, 256 chunks at a time
  for (int base = 0; base < g.n_chunks; base += DJ_JEC_SYNC_LANES) {
    const int c = base + lane;
    const int mine = c < g.n_chunks ? dj_je_clamp(chunks[c].blocks, 0, 8 * p.chunk_bytes + 8) : 0;
    part[lane] = mine;
    __syncthreads();
    for (int step = 1; step < DJ_JEC_SYNC_LANES; step <<= 1) {
      const int add = lane >= step ? part[lane - step] : 0;
      __syncthreads();
      part[lane] = min(part[lane] + add, 1 << 30);
      __syncthreads();
    }
    if (c < g.n_chunks) chunks[c].first_block = min(carry + part[lane] - mine, 1 << 30);
    __syncthreads();
    if (lane == 0) carry = min(carry + part[DJ_JEC_SYNC_LANES - 1], 1 << 30);
    __syncthreads();
  }
  if (lane == 0) {
    p.status[s] = 0;
    p.failing[s] = g.total;
    if (p.rounds) p.rounds[s] = rounds;
  }
}

// ---- final: one lane per chunk -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DJ_JE_LANES) void dj_jec_final_kernel(DjJecParams p) {
  __shared__ dj_je_row rows[8 * DJ_JE_LANES];
  __shared__ unsigned char natural[64];
  const int lane = threadIdx.x;
  const dj_je_row zero = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int r = 0; r < 8; ++r) rows[r * DJ_JE_LANES + lane] = zero;
  natural[lane] = dj_je_natural[lane];
  __syncthreads();      // the only barrier: lanes may leave behind it
  const long chunk = (long)blockIdx.x * DJ_JE_LANES + lane;
  if (chunk >= p.total_chunks) return;
  // the last segment whose first chunk is not behind this one
  int lo = 0, hi = p.n_segments - 1;
  for (int it = 0; it < 25 && lo < hi; ++it) {
    const int mid = lo + (hi - lo + 1) / 2;
    if ((long)p.seg[mid].reserved <= chunk) lo = mid;
    else hi = mid - 1;
  }
  const int s = lo;
  DjJecSegment g;
  dj_jec_segment(p, s, g);
  const long c = chunk - g.chunk_first;
  if (c < 0 || c >= g.n_chunks) return;
  const DjJecChunk* rec = p.chunks + chunk;
  DjJecState st = c == 0 ? dj_jec_unpack(g, 8 * g.begin, 0) : dj_jec_unpack(g, rec->entry_pos, rec->entry_state);
  const bool frozen = st.status != 0;
  const int first_block = dj_je_clamp(rec->first_block, 0, g.total);
  const long limit = c + 1 < g.n_chunks ? dj_jec_limit(g, (int)c, p.chunk_bytes) : 0x7FFFFFFFFFFFFFFFL;      // the last chunk has no end
  int blocks, failed;
  dj_jec_decode<true>(p, g, st, limit, blocks, first_block, reinterpret_cast<unsigned short*>(rows) + lane * 8, natural, failed);
  if (!frozen && failed >= 0 && failed < g.total) {      // at most one chunk of a segment gets here
    p.status[s] = st.status;
    p.failing[s] = failed;
  }
}

// ---- dc: predictors from differences, one workgroup per segment ------------------------------------------------------------------
__global__ __launch_bounds__(DJ_JEC_SYNC_LANES) void dj_jec_dc_kernel(DjJecParams p) {
  __shared__ unsigned part[DJ_JEC_SYNC_LANES];
  __shared__ unsigned carry;
  const int lane = threadIdx.x, s = blockIdx.x;
  DjJecSegment g;
  dj_jec_segment(p, s, g);
  const int failing = dj_je_clamp(p.failing[s], 0, g.total);
  const dj_je_row zero = {0u, 0u, 0u, 0u};
  for (int c = 0; c < g.ncomp; ++c) {
    const int nb = c == 0 ? g.nb[0] : c == 1 ? g.nb[1] : g.nb[2];
    const int u0 = c == 0 ? 0 : c == 1 ? g.nb[0] : g.nb[0] + g.nb[1];
    const int count = g.n_mcus * nb;      // the component's blocks in the segment, in scan order
    if (lane == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < count; base += DJ_JEC_SYNC_LANES) {      // uniform bounds
      const int j = base + lane;
      const int m = j / nb, u = u0 + j - m * nb;
      const int index = m * g.bpm + u;
      unsigned mine = 0;
      if (j < count && index < failing) {
        const long di = g.diff_first + index;
        if (di >= 0 && di < p.total_blocks) mine = (unsigned)(int)p.diffs[di];
      }
      part[lane] = mine;
      __syncthreads();
      for (int step = 1; step < DJ_JEC_SYNC_LANES; step <<= 1) {
        const unsigned add = lane >= step ? part[lane - step] : 0u;
        __syncthreads();
        part[lane] += add;
        __syncthreads();
      }
      if (j < count && index <= failing) {
        const long at = dj_jec_block_at(p, g, index, u);
        if (at >= 0) {
          if (index < failing) *reinterpret_cast<unsigned short*>(p.out + at) = (unsigned short)(carry + part[lane]);
          else
            for (int r = 0; r < 8; ++r) *reinterpret_cast<dj_je_row*>(p.out + at + 16 * r) = zero;
        }
      }
      __syncthreads();
      if (lane == 0) carry += part[DJ_JEC_SYNC_LANES - 1];
      __syncthreads();
    }
  }
}

static inline long dj_jec_round16(long v) { return (v + 15) / 16 * 16; }

extern "C" long dj_jpeg_entropy_chunked_scratch_bytes(long n_chunks, long n_files, long n_segments, long n_blocks) {
  return dj_jec_round16(32 * n_chunks) + dj_jec_round16(8 * n_files) + dj_jec_round16(4 * n_segments) + dj_jec_round16(2 * n_blocks);
}

extern "C" int dj_jpeg_entropy_decode_chunked(const unsigned char* bytes, long n_bytes, const dj_jpeg_entropy_desc* desc_dev,
                                              const dj_jpeg_entropy_desc* desc_host, int n_files,
                                              const dj_jpeg_entropy_seg* seg_dev, const dj_jpeg_entropy_seg* seg_host,
                                              int n_segments, const unsigned char* tables, int n_tables, unsigned char* out,
                                              long out_bytes, int* status, int chunk_bytes, unsigned char* scratch,
                                              long scratch_bytes, int* rounds, void* stream) {
  DJ_CHECK_ARG(bytes, "jpeg_entropy_decode_chunked: bytes is null");
  DJ_CHECK_ARG(desc_dev, "jpeg_entropy_decode_chunked: desc_dev is null");
  DJ_CHECK_ARG(desc_host, "jpeg_entropy_decode_chunked: desc_host is null");
  DJ_CHECK_ARG(seg_dev, "jpeg_entropy_decode_chunked: seg_dev is null");
  DJ_CHECK_ARG(seg_host, "jpeg_entropy_decode_chunked: seg_host is null");
  DJ_CHECK_ARG(tables, "jpeg_entropy_decode_chunked: tables is null");
  DJ_CHECK_ARG(out, "jpeg_entropy_decode_chunked: out is null");
  DJ_CHECK_ARG(status, "jpeg_entropy_decode_chunked: status is null");
  DJ_CHECK_ARG(scratch, "jpeg_entropy_decode_chunked: scratch is null");
  DJ_CHECK_ARG(n_files >= 1 && n_files <= 65535, "jpeg_entropy_decode_chunked: the number of files must be in 1..65535 (got %d)",
               n_files);
  DJ_CHECK_ARG(n_segments >= 1 && n_segments <= (1 << 24),
               "jpeg_entropy_decode_chunked: the number of segments must be in 1..2^24 (got %d)", n_segments);
  DJ_CHECK_ARG(n_tables >= 1 && n_tables <= 4 * 65535, "jpeg_entropy_decode_chunked: the number of tables must be in 1..262140 (got %d)",
               n_tables);
  DJ_CHECK_ARG(n_bytes >= 1 && out_bytes >= 1, "jpeg_entropy_decode_chunked: n_bytes / out_bytes must be >= 1");
  DJ_CHECK_ARG(chunk_bytes >= 16 && chunk_bytes <= 4096 && chunk_bytes % 16 == 0,
               "jpeg_entropy_decode_chunked: chunk_bytes must be a multiple of 16 in 16..4096 (got %d)", chunk_bytes);
  DJ_CHECK_ARG(((uintptr_t)out & 15) == 0 && ((uintptr_t)tables & 15) == 0 && ((uintptr_t)desc_dev & 7) == 0 &&
                   ((uintptr_t)seg_dev & 7) == 0 && ((uintptr_t)status & 3) == 0 && ((uintptr_t)scratch & 15) == 0 &&
                   ((uintptr_t)rounds & 3) == 0,
               "jpeg_entropy_decode_chunked: out, tables and scratch must be 16-byte, desc_dev and seg_dev 8-byte, status and "
               "rounds 4-byte aligned");
  int max_mcus = 0;
  const int rc = dj_je_check_records(desc_host, n_files, seg_host, n_segments, n_tables, n_bytes, out_bytes, &max_mcus);
  if (rc != DJ_OK) return rc;
  long total_chunks = 0, total_blocks = 0;
  int max_chunks = 0;
  for (int k = 0; k < n_segments; ++k) {
    const dj_jpeg_entropy_seg* sg = seg_host + k;
    const long n = (sg->end - sg->begin + chunk_bytes - 1) / chunk_bytes;
    const long chunks = n < 1 ? 1 : n;
    DJ_CHECK_ARG(chunks <= DJ_JEC_MAX_CHUNKS, "jpeg_entropy_decode_chunked: segment %d: %ld chunks of %d bytes, more than %d", k,
                 chunks, chunk_bytes, DJ_JEC_MAX_CHUNKS);
    DJ_CHECK_ARG(sg->reserved == total_chunks, "jpeg_entropy_decode_chunked: segment %d: its first chunk is %d in the record, %ld "
                 "by the segments in front of it", k, sg->reserved, total_chunks);
    total_chunks += chunks;
    DJ_CHECK_ARG(total_chunks <= 0x7FFFFFFFL - DJ_JE_LANES, "jpeg_entropy_decode_chunked: more than 2^31 chunks");
    if (chunks > max_chunks) max_chunks = (int)chunks;
  }
  for (int i = 0; i < n_files; ++i) {
    const dj_jpeg_entropy_desc* d = desc_host + i;
    int bpm = 0;
    for (int c = 0; c < d->n_components; ++c) bpm += d->h_blocks[c] * d->v_blocks[c];
    const long file_blocks = (long)d->mcus_x * d->mcus_y * bpm;
    DJ_CHECK_ARG(file_blocks <= (1L << 30), "jpeg_entropy_decode_chunked: file %d: %ld blocks, more than 2^30", i, file_blocks);
    total_blocks += file_blocks;
  }
  const long need = dj_jpeg_entropy_chunked_scratch_bytes(total_chunks, n_files, n_segments, total_blocks);
  DJ_CHECK_ARG(scratch_bytes >= need, "jpeg_entropy_decode_chunked: %ld bytes of scratch, %ld needed (%ld chunks, %d files, %d "
               "segments, %ld blocks)", scratch_bytes, need, total_chunks, n_files, n_segments, total_blocks);
  DjJecParams p;
  p.bytes = bytes;
  p.n_bytes = n_bytes;
  p.desc = desc_dev;
  p.n_files = n_files;
  p.seg = seg_dev;
  p.n_segments = n_segments;
  p.tables = tables;
  p.n_tables = n_tables;
  p.out = out;
  p.out_bytes = out_bytes;
  p.status = status;
  p.rounds = rounds;
  unsigned char* at = scratch;
  p.chunks = reinterpret_cast<DjJecChunk*>(at);
  at += dj_jec_round16(32 * total_chunks);
  p.file_first = reinterpret_cast<long*>(at);
  at += dj_jec_round16(8L * n_files);
  p.failing = reinterpret_cast<int*>(at);
  at += dj_jec_round16(4L * n_segments);
  p.diffs = reinterpret_cast<short*>(at);
  p.total_chunks = total_chunks;
  p.total_blocks = total_blocks;
  p.chunk_bytes = chunk_bytes;
  p.max_mcus = max_mcus;
  p.max_chunks = max_chunks;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(dj_jec_layout_kernel, dim3(1), dim3(DJ_JEC_SYNC_LANES), 0, st, p);
  DJ_CHECK_LAUNCH("dj_jpeg_entropy_decode_chunked (layout)");
  hipLaunchKernelGGL(dj_jec_zero_kernel, dim3((unsigned)n_files), dim3(DJ_JEC_SYNC_LANES), 0, st, p);
  DJ_CHECK_LAUNCH("dj_jpeg_entropy_decode_chunked (zero)");
  hipLaunchKernelGGL(dj_jec_sync_kernel, dim3((unsigned)n_segments), dim3(DJ_JEC_SYNC_LANES), 0, st, p);
  DJ_CHECK_LAUNCH("dj_jpeg_entropy_decode_chunked (sync)");
  hipLaunchKernelGGL(dj_jec_final_kernel, dim3((unsigned)dj_cdiv(total_chunks, DJ_JE_LANES)), dim3(DJ_JE_LANES), 0, st, p);
  DJ_CHECK_LAUNCH("dj_jpeg_entropy_decode_chunked (final)");
  hipLaunchKernelGGL(dj_jec_dc_kernel, dim3((unsigned)n_segments), dim3(DJ_JEC_SYNC_LANES), 0, st, p);
  DJ_CHECK_LAUNCH("dj_jpeg_entropy_decode_chunked (dc)");
  return DJ_OK;
}
