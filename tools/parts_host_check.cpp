// The phases of csrc/object_parts.hip replayed one after the other on the host, on ordinary memory, with the find / union core, the packed
// maximum and the keep rule of csrc/parts_core.h -- the functions the kernels run -- and compared with a flood fill over pixels.  A stand-alone
// program for a sanitizer run; it needs no GPU and no HIP:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I frtm-vos_amd/csrc tools/parts_host_check.cpp -o parts_host_check
//   ./parts_host_check
// It finds index and bound mistakes in the phase structure (tiles, seams, the pairs that are joined, the areas, the rule); it says nothing about
// concurrency: the kernels are held to the same reference on the GPU by tests/test_object_parts_gpu.py.
#include "parts_core.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

static const int TH = 32, TW = 64, NONE = 255, SLOTS = 16;      // FRTM_PARTS_TILE_H / _W of include/frtm_hip.h

struct Result {
  std::vector<int> comp;                    // name per pixel, -1 without a slot
  std::vector<unsigned char> labels;
  long long words[SLOTS][12];
};

struct Rule { int conn8; long long min_area; bool largest_only; int fill; };

static void begin_words(Result& R, int h, int w, int K, const std::vector<int>& ids, const Rule& rule) {
  for (int s = 0; s < SLOTS; ++s)
    for (int c = 0; c < 12; ++c) R.words[s][c] = 0;
  for (int s = 0; s < K; ++s) {
    R.words[s][5] = -1; R.words[s][6] = w; R.words[s][7] = h; R.words[s][8] = -1; R.words[s][9] = -1;
    R.words[s][10] = ids[s] != rule.fill; R.words[s][11] = ids[s];
  }
}

// from the names and areas of the parts to the words and the cleaned map: the contract, pixel by pixel
static void finish(Result& R, const std::vector<int>& slot, const std::vector<unsigned char>& input, const std::vector<int>& area_at_root, int h,
                   int w, int K, const std::vector<int>& ids, const Rule& rule) {
  begin_words(R, h, w, K, ids, rule);
  unsigned long long big[SLOTS] = {0};
  for (int p = 0; p < h * w; ++p)
    if (slot[p] != NONE && R.comp[p] == p) {
      R.words[slot[p]][0] += 1;
      R.words[slot[p]][2] += area_at_root[p];
      big[slot[p]] = std::max(big[slot[p]], pt_pack(area_at_root[p], p));
    }
  R.labels.assign((size_t)h * w, 0);
  for (int s = 0; s < K; ++s) { R.words[s][4] = pt_packed_area(big[s]); R.words[s][5] = pt_packed_name(big[s]); }
  for (int p = 0; p < h * w; ++p) {
    const int s = slot[p];
    if (s == NONE) { R.labels[p] = input[p]; continue; }
    const int r = R.comp[p], y = p / w, x = p % w;
    const bool keep = pt_keep(ids[s] != rule.fill, area_at_root[r], r, pt_packed_name(big[s]), rule.min_area, rule.largest_only);
    R.labels[p] = (unsigned char)(keep ? ids[s] : rule.fill);
    R.words[s][3] += keep;
    R.words[s][1] += keep && r == p;
    if (r == pt_packed_name(big[s])) {
      R.words[s][6] = std::min<long long>(R.words[s][6], x); R.words[s][7] = std::min<long long>(R.words[s][7], y);
      R.words[s][8] = std::max<long long>(R.words[s][8], x); R.words[s][9] = std::max<long long>(R.words[s][9], y);
    }
  }
}

// the reference: a flood fill from every pixel not yet named, in index order (so the seed is the name)
static Result flood(const std::vector<int>& slot, const std::vector<unsigned char>& input, int h, int w, int K, const std::vector<int>& ids,
                    const Rule& rule) {
  Result R;
  R.comp.assign((size_t)h * w, -1);
  std::vector<int> area((size_t)h * w, 0), stack;
  for (int p = 0; p < h * w; ++p) {
    if (slot[p] == NONE || R.comp[p] >= 0) continue;
    stack.assign(1, p);
    R.comp[p] = p;
    while (!stack.empty()) {
      const int q = stack.back(), y = q / w, x = q % w;
      stack.pop_back();
      area[p] += 1;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((dy == 0 && dx == 0) || (!rule.conn8 && dy != 0 && dx != 0)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
          const int n = yy * w + xx;
          if (slot[n] == slot[p] && R.comp[n] < 0) { R.comp[n] = p; stack.push_back(n); }
        }
    }
  }
  finish(R, slot, input, area, h, w, K, ids, rule);
  return R;
}

static bool gave_up = false;

// the kernels' phases
static Result phases(const std::vector<int>& slot, const std::vector<unsigned char>& input, int h, int w, int K, const std::vector<int>& ids,
                     const Rule& rule) {
  const int hw = h * w, tiles_x = (w + TW - 1) / TW, tiles_y = (h + TH - 1) / TH;
  std::vector<int> parent((size_t)hw, -1), area((size_t)hw, 0);
  // (1) local: per tile
  for (int t = 0; t < tiles_x * tiles_y; ++t) {
    const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
    std::vector<int> sl(TH * TW, NONE), lab(TH * TW), st(TH * TW), ln(TH * TW, 0), cnt(TH * TW, 0), rt(TH * TW, 0);
    for (int ly = 0; ly < TH; ++ly)
      for (int lx = 0; lx < TW; ++lx)
        if (y0 + ly < h && x0 + lx < w) sl[ly * TW + lx] = slot[(y0 + ly) * w + x0 + lx];
    for (int ly = 0; ly < TH; ++ly) {
      int start = 0;
      for (int lx = 0; lx < TW; ++lx) {
        const int me = ly * TW + lx;
        if (lx == 0 || sl[me - 1] != sl[me]) start = lx;
        st[me] = start;
        lab[me] = ly * TW + start;
        ln[ly * TW + start] += 1;
      }
    }
    for (int ly = 1; ly < TH; ++ly)
      for (int lane = 0; lane < TW; ++lane) {
        const int me = ly * TW + lane, up = me - TW, s = sl[me];
        if (s == NONE) continue;
        const bool first = st[me] == lane, last = lane == 63 || sl[me + 1] != s;
        if (sl[up] == s && (first || sl[up - 1] != s)) pt_union<PtPlain>(lab.data(), me, up, TH * TW, &gave_up);
        if (rule.conn8) {
          if (first && lane > 0 && sl[up - 1] == s) pt_union<PtPlain>(lab.data(), me, up - 1, TH * TW, &gave_up);
          if (last && lane < 63 && sl[up + 1] == s) pt_union<PtPlain>(lab.data(), me, up + 1, TH * TW, &gave_up);
        }
      }
    for (int me = 0; me < TH * TW; ++me) {
      if (sl[me] == NONE || st[me] != me % TW) continue;
      const int r = pt_find<PtPlain>(lab.data(), me, TH * TW, &gave_up);
      rt[me] = r;
      cnt[r] += ln[me];
    }
    for (int ly = 0; ly < TH; ++ly)
      for (int lane = 0; lane < TW; ++lane) {
        const int y = y0 + ly, x = x0 + lane, me = ly * TW + lane;
        if (y >= h || x >= w || sl[me] == NONE) continue;
        const int r = rt[me - lane + st[me]];
        parent[y * w + x] = (y0 + (r >> 6)) * w + x0 + (r & 63);
        area[y * w + x] = r == me ? cnt[me] : 0;
      }
  }
  // (2) seam: the threads of k_parts_seam, one after the other
  auto join = [&](int p, int s, int qy, int qx) {
    const int q = qy * w + qx;
    if (slot[q] == s) pt_union<PtPlain>(parent.data(), p, q, hw, &gave_up);
  };
  for (int t = 0; t < tiles_x * tiles_y; ++t) {
    const int y0 = (t / tiles_x) * TH, x0 = (t % tiles_x) * TW;
    for (int thread = 0; thread < 128; ++thread) {
      const int lane = thread & 63, wave = thread >> 6;
      int ly, lx;
      if (wave == 0) { ly = 0; lx = lane; }
      else { ly = 1 + (lane & 31); lx = lane < 32 ? 0 : TW - 1; }
      const int y = y0 + ly, x = x0 + lx;
      if (ly >= TH || y >= h || x >= w) continue;
      const int p = y * w + x, s = slot[p];
      if (s == NONE) continue;
      if (ly == 0) {
        if (y > 0) {
          join(p, s, y - 1, x);
          if (rule.conn8 && x > 0) join(p, s, y - 1, x - 1);
          if (rule.conn8 && x < w - 1) join(p, s, y - 1, x + 1);
        }
        if (lx == 0 && x > 0) join(p, s, y, x - 1);
      } else if (lx == 0) {
        if (x > 0) {
          join(p, s, y, x - 1);
          if (rule.conn8) join(p, s, y - 1, x - 1);
        }
      } else if (rule.conn8 && x < w - 1) {
        join(p, s, y - 1, x + 1);
      }
    }
  }
  // (3) flatten -- from the last pixel to the first, the order least like the order of the names
  for (int p = hw - 1; p >= 0; --p) {
    if (slot[p] == NONE) continue;
    const int r = pt_find<PtPlain>(parent.data(), p, hw, &gave_up);
    if (r == p) continue;
    parent[p] = r;
    if (area[p] > 0) area[r] += area[p];
  }
  Result R;
  R.comp = parent;
  finish(R, slot, input, area, h, w, K, ids, rule);      // (4), (5): sums, one maximum and the rule per pixel -- pt_pack and pt_keep
  return R;
}

static unsigned rng_state = 12345;
static unsigned rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// pictures of slots 0 .. K - 1 (NONE where `holes`)
static std::vector<int> picture(const std::string& what, int h, int w, int K) {
  std::vector<int> a((size_t)h * w, 0);
  auto at = [&](int y, int x) -> int& { return a[(size_t)y * w + x]; };
  const int o = K > 1 ? 1 : 0;
  if (what == "background") {
  } else if (what == "full") {
    std::fill(a.begin(), a.end(), o);
  } else if (what == "checker") {
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) at(y, x) = ((y + x) & 1) ? o : 0;
  } else if (what == "diagonal") {
    for (int y = 0; y < h; ++y) at(y, y % w) = o;
  } else if (what == "spiral") {
    int y0 = 0, x0 = 0, y1 = h - 1, x1 = w - 1;
    while (y0 <= y1 && x0 <= x1) {                       // rings two apart, each opened and joined to the next: one path
      for (int x = x0; x <= x1; ++x) at(y0, x) = o;
      for (int y = y0; y <= y1; ++y) at(y, x1) = o;
      for (int x = x0; x <= x1; ++x) at(y1, x) = o;
      for (int y = y0 + 2; y <= y1; ++y) at(y, x0) = o;
      if (y0 + 2 <= y1 && x0 + 1 <= x1) at(y0 + 2, x0 + 1) = o;
      if (y0 + 1 <= y1 && x0 < x1) at(y0 + 1, x0) = 0;
      y0 += 2; x0 += 2; y1 -= 2; x1 -= 2;
    }
  } else if (what == "comb" || what == "comb_mirrored") {
    for (int x = 0; x < w; x += 2) for (int y = 0; y < h; ++y) at(y, x) = o;
    for (int x = 0; x < w; ++x) at(what == "comb" ? h - 1 : 0, x) = o;                 // the joint: the last row, or the first
  } else if (what == "serpentine") {
    for (int y = 0; y < h; y += 2) {
      for (int x = 0; x < w; ++x) at(y, x) = o;
      if (y + 1 < h) at(y + 1, ((y / 2) & 1) ? 0 : w - 1) = o;
    }
  } else if (what == "ring") {
    const int cy = h / 2, cx = w / 2, R2 = std::min(h, w) / 2;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const int d2 = (y - cy) * (y - cy) + (x - cx) * (x - cx);
        if (d2 <= (R2 / 4) * (R2 / 4)) at(y, x) = (K > 2) ? 2 : o;
        else if (d2 >= (R2 * 3 / 4) * (R2 * 3 / 4) && d2 <= R2 * R2) at(y, x) = o;
      }
  } else if (what == "equal") {
    for (int y = 0; y < std::min(h, 3); ++y) for (int x = 0; x < std::min(w, 2); ++x) { at(y, x) = o; at(h - 1 - y, w - 1 - x) = o; }
  } else if (what == "corners") {
    at(0, 0) = at(0, w - 1) = at(h - 1, 0) = at(h - 1, w - 1) = o;
    for (int dy = -1; dy <= 0; ++dy) for (int dx = -1; dx <= 0; ++dx) if (TH + dy < h && TW + dx < w) at(TH + dy, TW + dx) = (dy == dx) ? o : 0;
  } else {                                               // noise: every pixel one of the K slots, or none
    for (auto& v : a) { const int r = (int)(rng() % (unsigned)(K + 1)); v = r == K ? NONE : r; }
    if (what == "noise2") for (auto& v : a) v = (rng() & 1) ? o : 0;
  }
  return a;
}

int main() {
  const int sizes[][2] = {{1, 1}, {1, 65}, {33, 1}, {2, 64}, {17, 63}, {63, 65}, {64, 64}, {65, 63}, {33, 130}, {129, 3}, {31, 63}, {32, 64},
                          {33, 65}, {97, 200}, {1, 300}, {300, 1}};
  const char* pictures[] = {"background", "full", "checker", "diagonal", "spiral", "comb", "comb_mirrored", "serpentine", "ring", "equal",
                            "corners", "noise", "noise2"};
  const Rule rules[] = {{0, 1, false, 0}, {1, 1, false, 0}, {0, 5, false, 0}, {1, 5, false, 0}, {0, 1, true, 0}, {1, 1, true, 0},
                        {0, 5, true, 7}, {1, 5, true, 7}};
  long long cases = 0, bad = 0;
  for (const auto& size : sizes)
    for (const char* what : pictures)
      for (int K : {1, 2, 5, 16})
        for (const Rule& rule : rules) {
          const int h = size[0], w = size[1];
          const std::vector<int> slot = picture(what, h, w, K);
          std::vector<int> ids(K);
          for (int s = 0; s < K; ++s) ids[s] = s == 0 ? 0 : (s == 1 && K > 2 ? 7 : 10 + s);
          std::vector<unsigned char> input((size_t)h * w);
          for (int p = 0; p < h * w; ++p) input[p] = slot[p] == NONE ? 200 : (unsigned char)ids[slot[p]];
          const Result a = flood(slot, input, h, w, K, ids, rule), b = phases(slot, input, h, w, K, ids, rule);
          bool same = a.comp == b.comp && a.labels == b.labels;
          for (int s = 0; s < SLOTS; ++s)
            for (int c = 0; c < 12; ++c) same = same && a.words[s][c] == b.words[s][c];
          ++cases;
          if (!same || gave_up) {
            ++bad;
            std::printf("MISMATCH %s %d x %d K %d conn8 %d min_area %lld largest %d fill %d gave_up %d\n", what, h, w, K, rule.conn8, rule.min_area,
                        (int)rule.largest_only, rule.fill, (int)gave_up);
            gave_up = false;
          }
        }
  std::printf("%lld cases, %lld mismatches\n", cases, bad);
  return bad ? 1 : 0;
}
