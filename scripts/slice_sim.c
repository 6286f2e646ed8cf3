// slice_sim.c -- dual_sim.c's host model of phase A with the lane count as a
// parameter (developer probe, not product): one DEFLATE block per workgroup
// of LANES lanes (LANES / 64 waves), each lane walking PER slices in lockstep
// (dual_sim's "512 slices" is 256 lanes x 2).  Per 64-lane wave: the
// speculative walk's length (max over the wave), then every sync iteration
// until no exit changes (a slice re-walks from its predecessor's latest exit
// until it meets a boundary of its speculative walk at symbols mf, 2mf, 4mf,
// 8mf -- mf = 2 under 400 bits -- or passes its stop), each costing the
// wave's longest re-walk; emit = spec.  Wave-steps per block = steps per wave
// x waves: what the CU's waves issue for one DEFLATE block.
// "first" is the first DEFLATE block of a BGZF block (the kernel's round 0),
// "second" every later one.  At 256 x 1 and 256 x 2 the figures equal
// dual_sim's (tests/test_slice_sim.py), whose two rows alternate DEFLATE block
// by DEFLATE block: the same over BGZF blocks of two.
// Also printed: the round-1 window (first symbol of the second block to the
// end of CDATA, in 16 B units, + 176 bits) over the file's blocks.
// Build: gcc -O2 -o scripts/bin/slice_sim scripts/slice_sim.c
// Run:   scripts/bin/slice_sim <C2-like BAM> [BGZF blocks] [lanes] [slices per lane]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const uint8_t LE[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const uint8_t DE[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const uint8_t CLO[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

static int g_pair = 1;
static const uint8_t* g_buf;
static uint64_t g_nbits;
static uint32_t bits(uint64_t p, int n) {  // n <= 24, LSB first
  uint32_t v = 0;
  for (int i = 0; i < n; ++i) {
    uint64_t q = p + i;
    uint32_t b = q < g_nbits ? (g_buf[q >> 3] >> (q & 7)) & 1 : 0;
    v |= b << i;
  }
  return v;
}

// canonical code: table of (symbol, length) indexed by reversed 15-bit code
typedef struct {
  int16_t sym[1 << 15];
  uint8_t len[1 << 15];
} Code;
static int build(Code* c, const uint8_t* lens, int n) {
  int cnt[16] = {0}, next[16];
  for (int i = 0; i < n; ++i) cnt[lens[i]]++;
  cnt[0] = 0;
  int code = 0;
  for (int l = 1; l < 16; ++l) {
    code = (code + cnt[l - 1]) << 1;
    next[l] = code;
  }
  memset(c->len, 0, sizeof c->len);
  for (int s = 0; s < n; ++s) {
    int l = lens[s];
    if (!l) continue;
    int cd = next[l]++;
    int rev = 0;
    for (int i = 0; i < l; ++i) rev |= ((cd >> i) & 1) << (l - 1 - i);
    for (int r = rev; r < (1 << 15); r += 1 << l) {
      c->sym[r] = s;
      c->len[r] = l;
    }
  }
  return 0;
}
static Code LIT, DIST, CL;

// one GPU symbol at p: returns bits consumed (0 = invalid / EOB); *eob set on EOB
static int step(uint64_t p, int* eob) {
  *eob = 0;
  uint32_t b = bits(p, 15);
  int l1 = LIT.len[b];
  if (!l1) return 0;
  int s = LIT.sym[b];
  if (s < 256) {
    if (g_pair && l1 < 10) {  // pair when the next literal code fits the 10-bit root too
      uint32_t b2 = bits(p + l1, 15);
      int l2 = LIT.len[b2];
      if (l2 && LIT.sym[b2] < 256 && l1 + l2 <= 10) return l1 + l2;
    }
    return l1;
  }
  if (s == 256) {
    *eob = 1;
    return l1;
  }
  if (s > 285) return 0;
  int n = l1 + LE[s - 257];
  uint32_t d = bits(p + n, 15);
  int dl = DIST.len[d];
  if (!dl || DIST.sym[d] >= 30) return 0;
  return n + dl + DE[DIST.sym[d]];
}


#define MAXSL 1024
static int LANES = 256, PER = 1, NSL = 256;  // lanes per DEFLATE block, slices per lane, slices
static double sp_cost[2], sy_cost[2], nwaves[2], sym_tot[2], iters[2], nblk[2];
static int cur_round = 0;
static int walkn(uint64_t g, uint64_t stop, uint64_t* pos, int cap) {
  int n = 0; uint64_t q = g;
  while (q < stop && n < cap) { int eob, k = step(q, &eob); if (!k || eob) break; q += k; pos[n++] = q; }
  return n;
}
// walk from g: symbols until reaching a checkpoint of the spec walk (merge) or
// passing stop; returns symbols walked, *ex = exit (first boundary >= stop)
static int sync_walk(uint64_t g, uint64_t stop, const uint64_t* sp, int ns, int mf, uint64_t sx, uint64_t* ex) {
  uint64_t q = g; int n = 0;
  for (;;) {
    for (int m = mf; m <= 8 * mf; m *= 2) if (m <= ns && sp[m - 1] == q) { *ex = sx; return n; }
    if (q >= stop) { *ex = q; return n; }
    int eob, k = step(q, &eob);
    if (!k || eob) { *ex = q; return n; }
    q += k; ++n;
  }
}
static uint64_t SPP[MAXSL][4096];
static void sim_sync(uint64_t b0, uint64_t bend) {
  uint64_t R = bend - b0, S = (R + NSL - 1) / NSL;
  int mf = S < 400 ? 2 : 4;
  static int ns[MAXSL], lenspec[MAXSL], cost[MAXSL];
  static uint64_t a_[MAXSL], st[MAXSL], sx[MAXSL], ex[MAXSL], prevx[MAXSL], start[MAXSL];
  const int W = LANES / 64;
  int nsl = 0;
  for (int sl = 0; sl < NSL; ++sl) {
    a_[sl] = b0 + sl * S;
    st[sl] = a_[sl] + S;
    if (a_[sl] >= bend) break;
    if (st[sl] > bend) st[sl] = bend;
    ns[sl] = walkn(a_[sl], st[sl], SPP[sl], 4096);
    sx[sl] = ns[sl] ? SPP[sl][ns[sl] - 1] : a_[sl];
    ex[sl] = sx[sl];  // the spec walk's exit: the first boundary >= stop
    lenspec[sl] = ns[sl];
    nsl = sl + 1;
  }
  for (int w = 0; w < W; ++w) {  // spec cost per wave
    int m = 0;
    for (int l = w * 64; l < w * 64 + 64; ++l)
      for (int k = 0; k < PER; ++k) {
        int sl = l + LANES * k;
        if (sl < nsl && lenspec[sl] > m) m = lenspec[sl];
      }
    sp_cost[cur_round] += m;
    nwaves[cur_round] += 1;
  }
  // sync iterations: slice i (> 0) re-walks from ex[i-1] when it differs from where its walk started
  for (int sl = 0; sl < nsl; ++sl) start[sl] = a_[sl];
  int it = 0;
  for (;;) {
    int any = 0;
    for (int sl = 0; sl < nsl; ++sl) prevx[sl] = ex[sl];
    for (int sl = 0; sl < nsl; ++sl) cost[sl] = 0;
    for (int sl = 1; sl < nsl; ++sl) {
      uint64_t px = prevx[sl - 1];
      if (px == start[sl]) continue;
      any = 1;
      start[sl] = px;
      uint64_t e;
      cost[sl] = sync_walk(px, st[sl], SPP[sl], ns[sl], mf, sx[sl], &e);
      ex[sl] = e;
    }
    if (!any || ++it > 40) break;
    for (int w = 0; w < W; ++w) {
      int m = 0;
      for (int l = w * 64; l < w * 64 + 64; ++l)
        for (int k = 0; k < PER; ++k) {
          int sl = l + LANES * k;
          if (sl < nsl && cost[sl] > m) m = cost[sl];
        }
      sy_cost[cur_round] += m;
    }
    iters[cur_round] += 1;
  }
  nblk[cur_round] += 1;
  for (int sl = 0; sl < nsl; ++sl) sym_tot[cur_round] += lenspec[sl];
}
static int cmp_u32(const void* a, const void* b) {
  uint32_t x = *(const uint32_t*)a, y = *(const uint32_t*)b;
  return x < y ? -1 : x > y;
}
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  int maxb = argc > 2 ? atoi(argv[2]) : 200;
  LANES = argc > 3 ? atoi(argv[3]) : 256;
  PER = argc > 4 ? atoi(argv[4]) : 1;
  NSL = LANES * PER;
  if (LANES < 64 || LANES % 64 || PER < 1 || NSL > MAXSL) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 1;
  fseek(f, 0, SEEK_END);
  long sz = ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* d = malloc(sz);
  if (fread(d, 1, sz, f) != (size_t)sz) return 1;
  long off = 0;
  int nb = 0, nwin = 0;
  uint32_t* win = malloc(sizeof(uint32_t) * (size_t)(maxb > 0 ? maxb : 1));
  unsigned long long dblocks = 0;
  while (off + 18 <= sz && nb < maxb) {
    int bsize = (d[off + 16] | (d[off + 17] << 8)) + 1;
    const uint8_t* cd = d + off + 18;
    uint64_t clen = bsize - 26;
    g_buf = cd;
    g_nbits = clen * 8;
    uint64_t abit = 8 * (uint64_t)((off + 18) & 15);  // CDATA's first bit, from the 16 B unit it lies in
    int nth = 0;
    uint64_t p = 0;
    ++nb;
    for (;;) {
      if (p + 3 > g_nbits) break;
      uint32_t h = bits(p, 3);
      p += 3;
      int fin = h & 1, type = h >> 1;
      if (type != 2) break;  // C2: dynamic blocks only
      int hlit = bits(p, 5) + 257, hdist = bits(p + 5, 5) + 1, hclen = bits(p + 10, 4) + 4;
      p += 14;
      uint8_t cl[19] = {0};
      for (int i = 0; i < hclen; ++i, p += 3) cl[CLO[i]] = bits(p, 3);
      build(&CL, cl, 19);
      uint8_t lens[320] = {0};
      int n = 0;
      while (n < hlit + hdist) {
        uint32_t b = bits(p, 15);
        int s = CL.sym[b];
        p += CL.len[b];
        if (s < 16) lens[n++] = s;
        else if (s == 16) { int r = 3 + bits(p, 2); p += 2; for (int i = 0; i < r; ++i, ++n) lens[n] = lens[n - 1]; }
        else if (s == 17) { int r = 3 + bits(p, 3); p += 3; n += r; }
        else { int r = 11 + bits(p, 7); p += 7; n += r; }
      }
      build(&LIT, lens, hlit);
      build(&DIST, lens + hlit, hdist);
      // true walk to EOB
      uint64_t q = p;
      for (;;) {
        int eob, k = step(q, &eob);
        if (!k) { fprintf(stderr, "bad symbol\n"); return 1; }
        q += k;
        if (eob) break;
      }
      cur_round = nth == 0 ? 0 : 1;
      if (nth == 1) {  // the round-1 window as the kernel stages it (a final second block: to the end of CDATA)
        uint64_t q0 = (abit + p) >> 7, q1 = ((abit + g_nbits + 176) >> 7) + 1;
        uint64_t qall = ((abit >> 3) + clen + 8 + 15) / 16 + 1;
        if (q1 > qall) q1 = qall;
        win[nwin++] = (uint32_t)((q1 - q0) * 16);
      }
      ++nth;
      sim_sync(p, q);
      ++dblocks;
      p = q;
      if (fin) break;
    }
    off += bsize;
  }
  printf("bgzf blocks %d, deflate blocks %llu, lanes %d x %d slices\n", nb, dblocks, LANES, PER);
  static const char* NAME[2] = {"first", "second"};
  for (int r = 0; r < 2; ++r) {
    if (nblk[r] == 0) continue;
    double sp = sp_cost[r] / nwaves[r], sy = sy_cost[r] / nwaves[r];
    printf("DEFLATE block %s, %d lanes x %d: per wave spec %.1f  sync (all iterations) %.1f  emit %.1f  total %.1f; "
           "wave-steps per block %.1f; sync iterations per block %.2f, symbols/slice %.1f\n", NAME[r], LANES, PER, sp, sy,
           sp, 2 * sp + sy, (2 * sp + sy) * (LANES / 64), iters[r] / nblk[r], sym_tot[r] / (nblk[r] * NSL));
  }
  if (nwin) {
    qsort(win, nwin, sizeof(uint32_t), cmp_u32);
    static const uint32_t CAP[2] = {8368, 12464};  // the stage at 16 KB and at 20 KB of LDS
    int over[2] = {0, 0};
    for (int i = 0; i < nwin; ++i)
      for (int k = 0; k < 2; ++k) over[k] += win[i] > CAP[k];
    printf("round-1 window bytes over %d blocks: p1 %u  p50 %u  p99 %u  max %u; over %u B: %.4f  over %u B: %.4f\n", nwin,
           win[nwin / 100], win[nwin / 2], win[(int)(nwin * 0.99)], win[nwin - 1], CAP[0], (double)over[0] / nwin, CAP[1],
           (double)over[1] / nwin);
  }
  return 0;
}
