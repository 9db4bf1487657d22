// Which kernel form each conv of the ResNet trunk takes, and which weight images it therefore holds: ONE decision, in plain C++ (no HIP header, no
// allocation, no environment variable), asked by run_conv() for every launch and by frtm_backbone_conv_route() without a device (csrc/backbone.hip).
#pragma once
#include <algorithm>
#include "../../include/frtm_hip.h"

struct TrunkConv {
  int Cout, Cin, ks, stride, pad;
  // per-conv launch plan (frtm_backbone_set_conv_plan; 0 = the planner's choice): the GEMM tile of the path the conv takes (direct 1x1 /
  // gather conv, or the batched products of the three-launch Winograd forms; the output block 1..3 of the fused F(2x2,3x3) kernel) and split-K
  int plan_tile = 0, plan_splitk = 0;
};

// The switches of a trunk handle (the setters of include/frtm_hip.h; frtm_backbone_create reads the environment into the three marked fields)
struct TrunkModes {
  bool winograd = true;
  int winograd4 = 2;           // three-launch Winograd where it is eligible: 0 = off, 1 = F(4x4,3x3) only, 2 = F(4x4,3x3) or F(6x6,3x3), whichever has fewer products (FRTM_NO_WINO4 / FRTM_NO_WINO6)
  // fewest 64x64 product tiles for which the three-launch forms are taken (256 = one per CU: measured at batch 1 -- the streaming path -- 2.49 -> 2.23 ms per trunk pass; FRTM_WINO4_MIN_TILES)
  int wino4_min_tiles = 256;
  int precision = 0;           // frtm_backbone_set_precision / _set_bf16_pieces: 0 = fp32, 1 = bf16x3, 2 = bf16x1 for the stride-1 1x1 convs that kTrunkRules routes
  // FRTM_BF16X1_MIN_COLS=n (tests and measurements on small frames): a bf16x1 trunk routes EVERY eligible conv from n columns per launch on, instead of the measured table
  int bf16x1_min_cols = -1;
  bool bf16x1_3x3 = false;     // frtm_backbone_set_bf16x1_3x3: with precision == 2, the routed 3x3 convs on bf16 MFMAs as well; stored whatever the precision is
  bool bf16_act = false;       // frtm_backbone_set_bf16_act: with precision == 2 && bf16x1_3x3, bf16 storage of the tensors only bf16 kernels touch (act_plan); stored whatever the others are
};

// The convs a reduced-precision trunk sends to a bf16 kernel, per layout: FRTM_WLAYOUT_BF16X3 (csrc/conv_bf16x3.hip) and _BF16X1 (csrc/conv_bf16x1.hip)
// for stride-1 1x1 convs, _BF16X1_3X3 (csrc/conv3x3_bf16x1.hip) and _BF16X1_3X3_S2 (csrc/conv3x3s2_bf16x1.hip) for 3x3 pad-1 convs of stride 1 and 2.
// A shape is routed only where the bf16 median measured faster than the fp32 form the conv would otherwise take (Winograd F(6x6) / F(4x4) / F(2x2), the
// halo kernel for stride 2, the fp32 GEMM for 1x1) by more than the spread (max - min over the alternating rounds) of the fp32 arm in the same run, per
// shape and columns of the launch, on 480x854 frames at 1 and 8 frames per launch.  A shape faster at 8 frames only is routed from its 8-frame column
// count on; one faster at 1 frame as well, from its 1-frame column count on.  Shapes that were not measured (the conv1 of a bottleneck stage's first
// block: 64 -> 64, 256 -> 128, 512 -> 256, 1024 -> 512), or were not faster, stay fp32.
// The 3x3 images are bf16 [Cin/16][9][2][Mp][8], 18 Cin Cout bytes per conv -- every 3x3 conv of ResNet-101 (3 x 64^2 + 4 x 128^2 + 23 x 256^2 +
// 3 x 512^2 weights x 18 B) comes to about 43 MB of device memory; only the convs the table (or FRTM_BF16X1_MIN_COLS) can route are packed.
struct TrunkRule { int layout, Cin, Cout, stride; long min_cols; };
static const TrunkRule kTrunkRules[] = {
  // bf16x3 (profiles/bf16x3_trunk_time.txt): layer4's conv3 only, with at least 3240 columns in the launch (8 frames: 61 against
  // 69 us).  Every other trunk 1x1 shape, and this one at 1 frame, measured slower (0.27-0.98x).
  {FRTM_WLAYOUT_BF16X3, 512, 2048, 1, 3240},
  // bf16x1 (tools/bf16x1_trunk_time.py -> profiles/bf16x1_trunk_time.txt); us per launch, fp32 / bf16x1 (automatic tile form):  1 frame          8 frames
  {FRTM_WLAYOUT_BF16X1, 256, 1024, 1, 1620},      // layer3 conv3, 30x54                                  13.3 / 10.0      58.6 / 41.1
  {FRTM_WLAYOUT_BF16X1, 1024, 256, 1, 1620},      // layer3 conv1                                         18.8 / 15.1      67.5 / 24.7
  {FRTM_WLAYOUT_BF16X1, 128, 512, 1, 6420},       // layer2 conv3, 60x107                                 14.2 / 11.4      67.6 / 65.0
  {FRTM_WLAYOUT_BF16X1, 512, 128, 1, 6420},       // layer2 conv1                                         13.9 / 11.0      56.7 / 31.9
  {FRTM_WLAYOUT_BF16X1, 512, 2048, 1, 405},       // layer4 conv3, 15x27                                  20.4 / 11.6      71.9 / 33.3
  {FRTM_WLAYOUT_BF16X1, 2048, 512, 1, 3240},      // layer4 conv1: slower at 1 frame                      22.3 / 27.6      92.3 / 33.6
  {FRTM_WLAYOUT_BF16X1, 256, 64, 1, 25680},       // layer1 conv1, 120x214                                13.2 /  9.7      59.8 / 48.1
  // 64 -> 256 (layer1 conv3 and downsample, K = 64: one chunk, nothing to pipeline)                      14.2 / 17.2     114.7 / 139.1: stays fp32
  // bf16x1_3x3 (tools/bf16x1_trunk3x3_time.py -> profiles/bf16x1_trunk3x3_time.txt); us per launch, fp32 form / bf16 (automatic tile form):
  {FRTM_WLAYOUT_BF16X1_3X3, 64, 64, 1, 25680},    // layer1, 120x214, fused F(2x2)                        15.2 / 11.3      77.2 / 30.2
  {FRTM_WLAYOUT_BF16X1_3X3, 128, 128, 1, 6420},   // layer2, 60x107, F(6x6)                               24.0 / 16.7      70.8 / 23.5
  {FRTM_WLAYOUT_BF16X1_3X3, 256, 256, 1, 12960},  // layer3, 30x54, F(6x6): slower at 1 frame             22.0 / 28.4      57.3 / 30.4
  {FRTM_WLAYOUT_BF16X1_3X3, 512, 512, 1, 3240},   // layer4, 15x27, F(4x4): slower at 1 frame             31.1 / 50.6      62.4 / 51.6
  {FRTM_WLAYOUT_BF16X1_3X3_S2, 128, 128, 2, 6420},    // ResNet-50 / 101 layer2 opener, -> 60x107, halo   40.2 / 31.5     193.8 / 52.1
  {FRTM_WLAYOUT_BF16X1_3X3_S2, 256, 256, 2, 12960},   // ... layer3 opener, -> 30x54: slower at 1 frame   45.3 / 56.7     203.0 / 58.0
  {FRTM_WLAYOUT_BF16X1_3X3_S2, 512, 512, 2, 3240},    // ... layer4 opener, -> 15x27: slower at 1 frame   49.7 / 101.7    201.0 / 102.1
  {FRTM_WLAYOUT_BF16X1_3X3_S2, 64, 128, 2, 6420},     // ResNet-18 / 34 layer2 opener, -> 60x107, halo    30.5 / 18.3     105.2 / 29.8
  {FRTM_WLAYOUT_BF16X1_3X3_S2, 128, 256, 2, 1620},    // ... layer3 opener, -> 30x54                      31.8 / 30.8     107.1 / 32.3
  {FRTM_WLAYOUT_BF16X1_3X3_S2, 256, 512, 2, 3240},    // ... layer4 opener, -> 15x27: slower at 1 frame   34.4 / 53.2     103.6 / 53.9
};

// Fewest columns (B x Ho x Wo) of a launch from which `layout`, one of the four bf16 layouts, takes conv c; -1: never, the conv holds no such image.
// The geometry is what the layout's kernel accepts; FRTM_BF16X1_MIN_COLS replaces the table for the bf16x1 layouts (6, 7, 8), not for bf16x3.
static inline long bf16_min_cols(const TrunkModes& m, const TrunkConv& c, int layout) {
  const bool one = layout == FRTM_WLAYOUT_BF16X3 || layout == FRTM_WLAYOUT_BF16X1;
  if (one ? !(c.ks == 1 && c.stride == 1 && c.pad == 0 && c.Cin % 16 == 0)
          : !(c.ks == 3 && c.pad == 1 && c.stride == (layout == FRTM_WLAYOUT_BF16X1_3X3_S2 ? 2 : 1))) return -1;
  if (layout != FRTM_WLAYOUT_BF16X3 && m.bf16x1_min_cols >= 0) return m.bf16x1_min_cols;
  for (const TrunkRule& r : kTrunkRules)
    if (r.layout == layout && r.Cin == c.Cin && r.Cout == c.Cout && r.stride == c.stride) return r.min_cols;
  return -1;
}

// the image of the direct form: the halo image for 3x3 pad-1 convs of stride 1 or 2, the GEMM image otherwise
static inline int base_layout(const TrunkConv& c) { return (c.ks == 3 && c.stride <= 2 && c.pad == 1) ? FRTM_WLAYOUT_HALO3X3 : FRTM_WLAYOUT_GEMM; }

// Bit mask over FRTM_WLAYOUT_* 0..8: the weight images a loaded conv holds under modes m.  The fp32 images always (the Winograd ones for 3x3 stride-1
// pad-1 convs, F(4x4) / F(6x6) for the wide ones); a bf16 image once its mode has been on -- `have`, the images the conv holds now, keeps those.
static inline unsigned wanted_images(const TrunkModes& m, const TrunkConv& c, unsigned have = 0) {
  unsigned want = 1u << base_layout(c);
  if (c.ks == 3 && c.stride == 1 && c.pad == 1) {
    want |= 1u << FRTM_WLAYOUT_WINO3X3;
    if (c.Cin >= 128 && c.Cin % 32 == 0 && c.Cout % 64 == 0) want |= 1u << FRTM_WLAYOUT_WINO4 | 1u << FRTM_WLAYOUT_WINO6;
  }
  for (int l = FRTM_WLAYOUT_BF16X3; l <= FRTM_WLAYOUT_BF16X1_3X3_S2; ++l) {
    const bool on = l == FRTM_WLAYOUT_BF16X3 ? m.precision == 1 : l == FRTM_WLAYOUT_BF16X1 ? m.precision == 2 : m.bf16x1_3x3;
    if (bf16_min_cols(m, c, l) >= 0 && (on || (have >> l & 1))) want |= 1u << l;
  }
  return want;
}

// The planner's exceptions from the IN-TRUNK tile scan (tools/trunk_tile_scan.py, profiles/r04_trunk_tile_scan.txt: every candidate tile
// of every conv class timed as a whole RN101 pass with the tracker's lanes).  At 16 frames in two lanes NO class moves the pass by more
// than the run-to-run noise (+0.2 % for the whole scanned plan: the concurrent lane fills the tails that separate the tiles when a launch
// is timed alone, profiles/r03_g32p_bench.txt); at the 4-5 frames per lane of the first-frame pass the 32x32x2-MFMA kernel is ahead on the
// two dominant layer3 GEMMs (9.08 -> 8.92 ms per 9-frame pass).
// `products`: the launch is the batched GEMM of a three-launch Winograd form (the tile of a 3x3 conv's DIRECT form is never touched).
static inline int scanned_tile(const TrunkConv& c, int B, int Ho, int Wo, bool products) {
  // Round 5, the exception itself A/B-ed (three alternating runs on one box, tools/trunk_bench.py): 9 frames in two lanes (102 / 127 column tiles per lane)
  // 8.98-9.03 ms with it against 9.09-9.25 without; 5 frames (51 / 76 tiles) 5.79-5.80 with against 5.69-5.72 without -> from 96 tiles on only.
  const long ntiles = ((long)B * Ho * Wo + 63) / 64;
  if (ntiles < 96 || ntiles > 130 || c.Cin != 256) return 0;
  if (products) return (c.ks == 3 && c.stride == 1 && c.Cout == 256) ? FRTM_TILE_G32_64x64 : 0;            // (tile counts are padded to 64)
  if (c.ks == 1 && c.stride == 1 && c.Cout == 1024 && ((long)Ho * Wo) % 4 == 0) return FRTM_TILE_G32_64x64;  // (dwordx4 staging needs H*W % 4 == 0)
  return 0;
}

static inline int conv_out_dim(const TrunkConv& c, int in, int pad) { return (in + 2 * pad - c.ks) / c.stride + 1; }
// algorithmic (direct-form) FLOPs of one launch
static inline double direct_flops(const TrunkConv& c, int B, int Ho, int Wo) { return 2.0 * c.Cout * (double)B * Ho * Wo * c.Cin * c.ks * c.ks; }

struct Route {
  int layout;          // FRTM_WLAYOUT_*: the kernel form, and the image it reads
  int tile, splitk;    // frtm_conv_desc.tile / .splitk
  int flops_slot;      // frtm_backbone_last_flops_form: 0 direct (the bf16 forms included: full MACs), 1 F(2x2,3x3), 2 F(4x4,3x3), 3 F(6x6,3x3)
  double exec_flops;   // the launch at the MACs it executes (F(2x2,3x3): 16 per 2x2 outputs instead of 36; F(4x4,3x3): 36 per 4x4 tile instead of 144, partial edge tiles included)
  size_t ws4_elems;    // floats of transformed input + product tensors the three-launch forms need (0: the form takes the split-K workspace, or none)
};

// The form of one launch: conv c on B images with Ho x Wo outputs under padding `pad` (the conv's own, or 0 for the stem on its pre-padded image),
// `have` = the images it holds (wanted_images() for a loaded conv).  A per-conv plan keeps its conv fp32.
static inline Route choose_route(const TrunkModes& m, const TrunkConv& c, int B, int Ho, int Wo, int pad, unsigned have) {
  const auto has = [&](int layout) { return (have >> layout & 1) != 0; };
  const long cols = (long)B * Ho * Wo;
  const auto bf16 = [&](int layout) {
    const long min_cols = bf16_min_cols(m, c, layout);
    return has(layout) && !c.plan_tile && !c.plan_splitk && min_cols >= 0 && cols >= min_cols;
  };
  const double direct = direct_flops(c, B, Ho, Wo);
  Route r = {base_layout(c), 0, 1, 0, direct, 0};
  // bf16x1_3x3 trunks: the routed 3x3 convs on bf16 MFMAs (direct form: full MACs), before any Winograd form is considered
  const int l3 = c.stride == 2 ? FRTM_WLAYOUT_BF16X1_3X3_S2 : FRTM_WLAYOUT_BF16X1_3X3;
  if (m.precision == 2 && m.bf16x1_3x3 && pad == 1 && bf16(l3)) { r.layout = l3; return r; }
  // Winograd F(4x4,3x3) / F(6x6,3x3), three-launch form (conv_wino4.hip), for the wide 3x3 stride-1 convs: 2.25 / 1.78 multiplications
  // per output instead of 4; eligible when the products fill the chip as one GEMM launch and the output tiles waste < 25 % on the
  // map's edges; of the two, the form with fewer products = (m+2)^2 x padded tile count (30x54: 6x6 tiles fit exactly, 64 x 384 against
  // 36 x 896 at 8 frames).  Measured at 8 frames (tools/wino4_bench.py): 256 ch 30x54 62 (F6) / 69 (F4) vs 100 us fused F(2x2), 512 ch
  // 15x27 58 / 68 vs 105, 128 ch 60x107 76 / 85 vs 101; 64 ch 120x214 is slower (128 / 145 vs 108: K = 64 GEMMs, transform traffic).
  if (has(FRTM_WLAYOUT_WINO4) && m.winograd && m.winograd4) {
    long best_cost = 0;
    for (int fm : {6, 4}) {
      if (fm == 6 && (m.winograd4 < 2 || !has(FRTM_WLAYOUT_WINO6))) continue;
      const int th = (Ho + fm - 1) / fm, tw = (Wo + fm - 1) / fm, NP = (fm + 2) * (fm + 2);
      const long T = (long)B * th * tw, Tp = (T + 63) / 64 * 64;
      if ((long)((c.Cout + 63) / 64) * (NP * Tp / 64) < m.wino4_min_tiles || (long)fm * fm * th * tw * 4 > (long)5 * Ho * Wo ||
          (size_t)NP * std::max(c.Cin, c.Cout) * Tp * 4 >= 0x7fffffffull)       // (32-bit buffer offsets of the transformed tensors)
        continue;
      if (r.ws4_elems && NP * Tp >= best_cost) continue;
      best_cost = NP * Tp;
      r.layout = fm == 6 ? FRTM_WLAYOUT_WINO6 : FRTM_WLAYOUT_WINO4;
      r.flops_slot = fm == 6 ? 3 : 2;
      r.exec_flops = 2.0 * c.Cout * (double)c.Cin * NP * (double)T;
      r.ws4_elems = (size_t)NP * (c.Cin + c.Cout) * Tp;
    }
    if (r.ws4_elems) {
      r.tile = c.plan_tile ? c.plan_tile : scanned_tile(c, B, Ho, Wo, true);
      return r;
    }
  }
  // Winograd for the 3x3 stride-1 convs whenever the launch has enough 8x8 output blocks to fill the chip without split-K
  if (has(FRTM_WLAYOUT_WINO3X3) && m.winograd && (long)B * ((Ho + 7) / 8) * ((Wo + 7) / 8) * ((c.Cout + 31) / 32) >= FRTM_WINO_MIN_BLOCKS) {
    r.layout = FRTM_WLAYOUT_WINO3X3;
    r.tile = (c.plan_tile >= 1 && c.plan_tile <= 3) ? c.plan_tile : 0;
    r.flops_slot = 1;
    r.exec_flops = direct * (16.0 / 36.0);
    return r;
  }
  if (m.precision == 1 && bf16(FRTM_WLAYOUT_BF16X3)) { r.layout = FRTM_WLAYOUT_BF16X3; return r; }
  if (m.precision == 2 && bf16(FRTM_WLAYOUT_BF16X1)) { r.layout = FRTM_WLAYOUT_BF16X1; return r; }
  r.tile = c.plan_tile ? c.plan_tile : scanned_tile(c, B, Ho, Wo, false);
  r.splitk = c.plan_splitk;
  return r;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// The bf16x1_act mode: the stored format of every tensor of the block walk (csrc/backbone.hip: forward_lane), FRTM_ACT_FP32 or FRTM_ACT_BF16.
// ---------------------------------------------------------------------------------------------------------------------------------------------
struct TrunkBlock { int conv[3]; int nconv; int ds; };   // conv indices of a residual block (ds = -1: identity shortcut)
struct ActFmt { int in, res, out; };                     // FRTM_ACT_* of one conv's input, residual and output

// fmt[i] for each of the n convs of a trunk (convs[i], `have[i]` = the images it holds: choose_route's argument) in one pass of B frames per lane at
// H x W.  A tensor is bf16 exactly when the mode is in effect (bf16_act with precision == 2 && bf16x1_3x3), its channel count is a multiple of 8,
// its producer is routed to layout 6, 7 or 8 at that launch and so is every conv that reads it, as input or as residual.  That can hold for a
// block's t1 (conv1 -> conv2) and t2 (conv2 -> conv3), for a downsample output (-> the last conv's residual) and for a block output that does not
// end a stage (-> the next block's conv1, its downsample if it has one, else its last conv's residual).  The pool output and every stage output --
// every tap, wanted or not -- stay fp32, and so does whatever an fp32 form reads or writes.
static inline void act_plan(const TrunkModes& m, const TrunkConv* const* convs, const unsigned* have, int n, const TrunkBlock* const stage[4],
                            const int nblocks[4], int B, int H, int W, ActFmt* fmt) {
  for (int i = 0; i < n; ++i) fmt[i] = {FRTM_ACT_FP32, FRTM_ACT_FP32, FRTM_ACT_FP32};
  if (!(m.bf16_act && m.precision == 2 && m.bf16x1_3x3)) return;
  int ch = conv_out_dim(*convs[0], H, convs[0]->pad), cw = conv_out_dim(*convs[0], W, convs[0]->pad);      // the stem, then the 3x3 stride-2 pad-1 pool
  ch = (ch + 2 - 3) / 2 + 1; cw = (cw + 2 - 3) / 2 + 1;
  // is conv idx on h x w inputs a bf16x1 launch?  (h, w become its output size)
  const auto routed = [&](int idx, int& h, int& w) {
    const TrunkConv& c = *convs[idx];
    h = conv_out_dim(c, h, c.pad); w = conv_out_dim(c, w, c.pad);
    const int l = choose_route(m, c, B, h, w, c.pad, have[idx]).layout;
    return l == FRTM_WLAYOUT_BF16X1 || l == FRTM_WLAYOUT_BF16X1_3X3 || l == FRTM_WLAYOUT_BF16X1_3X3_S2;
  };
  for (int s = 0; s < 4; ++s) {
    bool x_bf16 = false;                        // the block's input: a stage begins on the pool output or a stage output
    // routed flags of block b's convs (r[0 .. nconv - 1], r[3] = its downsample), worked out one block ahead: a block output asks its readers
    bool r[4] = {}, rn[4] = {};
    const auto block_routes = [&](const TrunkBlock& bl, bool* out, int& h, int& w) {
      int hd = h, wd = w;
      out[3] = bl.ds >= 0 && routed(bl.ds, hd, wd);
      for (int k = 0; k < bl.nconv; ++k) out[k] = routed(bl.conv[k], h, w);
    };
    if (nblocks[s] > 0) block_routes(stage[s][0], r, ch, cw);
    for (int b = 0; b < nblocks[s]; ++b) {
      const TrunkBlock& bl = stage[s][b];
      const int last = bl.conv[bl.nconv - 1];
      const bool ends_stage = b + 1 == nblocks[s];
      if (!ends_stage) block_routes(stage[s][b + 1], rn, ch, cw);
      fmt[bl.conv[0]].in = x_bf16;
      for (int k = 0; k + 1 < bl.nconv; ++k) {                      // t1, t2
        const bool bf = r[k] && r[k + 1] && convs[bl.conv[k]]->Cout % 8 == 0;
        fmt[bl.conv[k]].out = fmt[bl.conv[k + 1]].in = bf;
      }
      if (bl.ds >= 0) {
        const bool bf = r[3] && r[bl.nconv - 1] && convs[bl.ds]->Cout % 8 == 0;
        fmt[bl.ds].in = x_bf16;
        fmt[bl.ds].out = fmt[last].res = bf;
      } else fmt[last].res = x_bf16;
      bool out_bf16 = false;
      if (!ends_stage) {
        const TrunkBlock& nx = stage[s][b + 1];
        out_bf16 = r[bl.nconv - 1] && rn[0] && (nx.ds >= 0 ? rn[3] : rn[nx.nconv - 1]) && convs[last]->Cout % 8 == 0;
      }
      fmt[last].out = out_bf16;
      x_bf16 = out_bf16;
      for (int k = 0; k < 4; ++k) r[k] = rn[k];
    }
  }
}
