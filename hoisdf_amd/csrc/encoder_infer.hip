// The image encoder (hoisdf_amd/nets/encoder.py: ResNet backbone + top-down decoder) in evaluation mode as prepare + ONE call that
// only enqueues: image in, the five pyramid levels (and the three auxiliary maps) out, on the convolution of conv.hip.  Exact f32,
// forward only: no training-mode statistics, no backward.
// One walk of the module structure (build_net) serves the tensor table (checkpoint keys in state_dict() order), the blob layout, the
// workspace carving and the launch sequence, so they cannot drift apart.
//   prepare: every BatchNorm folded into its convolution from the running statistics (eps = 1e-5, nn.BatchNorm2d's default, which is
//            what encoder.py builds), every weight packed to [ky][kx][ci][co]; nothing of it is redone per frame.
//   infer:   stem -> maxpool -> the residual stages (residual add + ReLU in the last convolution's epilogue) -> 1x1 reductions and
//            transposed convolutions writing channel slices of one map (torch.cat) -> 3x3 fuse convolutions -> the aux heads.
#include <map>
#include <string>
#include <vector>

#include "common.h"

namespace hoisdf {
namespace {

constexpr float BN_EPS = 1e-5f;

struct EncTensor {
  std::string name;
  long numel;
};
struct EncLayer {
  int cin, cout, k, stride, pad, transposed;
  int t_w, t_b, t_bn;      // tensor indices: weight, bias (-1: none), BatchNorm weight (-1: none; bias / mean / var follow it)
  long w_off, b_off;       // float offsets in the prepared blob
};
struct EncBlock {
  int c1, c2, c3, ds;      // layer ids (c3 = -1: basic block; ds = -1: identity skip)
};
struct EncNet {
  std::vector<EncTensor> tensors;
  std::vector<EncLayer> layers;
  bool bottleneck, deep, big;
  int stem;
  std::vector<EncBlock> stage[4];
  int planes[4], oc[4];              // per stage: block width, output channels
  int c0d, cd[4], dc[4], cf[4];      // decoder: stride-32 reduction, skip reductions (-1: none), transposed convs, fuse convs
  int rc[4], dco[4], fo[4];          // channels: reduced skip (= raw skip without a reduction), transposed-conv output, fused output
  std::vector<int> head[3];
  long blob_floats;
};

long round64(long n) { return (n + 63) & ~63L; }

int add_conv(EncNet& n, const std::string& key, int cin, int cout, int k, int stride, int pad, bool bias, bool transposed = false) {
  EncLayer l{};
  l.cin = cin; l.cout = cout; l.k = k; l.stride = stride; l.pad = pad; l.transposed = transposed;
  l.t_w = (int)n.tensors.size();
  n.tensors.push_back({key + ".weight", (long)cin * cout * k * k});
  l.t_b = -1;
  if (bias) {
    l.t_b = (int)n.tensors.size();
    n.tensors.push_back({key + ".bias", (long)cout});
  }
  l.t_bn = -1;
  l.w_off = n.blob_floats;
  n.blob_floats += round64((long)k * k * cin * ((cout + 3) & ~3));
  l.b_off = n.blob_floats;
  n.blob_floats += round64((cout + 3) & ~3);
  n.layers.push_back(l);
  return (int)n.layers.size() - 1;
}
void add_bn(EncNet& n, int layer, const std::string& key) {
  n.layers[layer].t_bn = (int)n.tensors.size();
  const long c = n.layers[layer].cout;
  for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) n.tensors.push_back({key + s, c});
}
// nets/encoder.py _convs: Conv(+BN+ReLU) chain, Sequential indices 3 i / 3 i + 1
std::vector<int> add_convs(EncNet& n, const std::string& key, const std::vector<int>& dims, int k, int pad, bool bnrelu_final) {
  std::vector<int> ids;
  int idx = 0;
  for (size_t i = 0; i + 1 < dims.size(); ++i) {
    const int id = add_conv(n, key + "." + std::to_string(idx), dims[i], dims[i + 1], k, 1, pad, true);
    ids.push_back(id);
    ++idx;
    if (i + 2 < dims.size() || bnrelu_final) {
      add_bn(n, id, key + "." + std::to_string(idx));
      idx += 2;
    }
  }
  return ids;
}
int add_deconv(EncNet& n, const std::string& key, int cin, int cout) {
  const int id = add_conv(n, key + ".0", cin, cout, 4, 2, 1, false, true);
  add_bn(n, id, key + ".1");
  return id;
}

void build_net(int resnet_type, int big, EncNet& n) {
  static const int counts[5][4] = {{2, 2, 2, 2}, {3, 4, 6, 3}, {3, 4, 6, 3}, {3, 4, 23, 3}, {3, 8, 36, 3}};
  const int which = resnet_type == 18 ? 0 : resnet_type == 34 ? 1 : resnet_type == 50 ? 2 : resnet_type == 101 ? 3 : 4;
  n.bottleneck = resnet_type >= 50;
  n.deep = resnet_type >= 50;
  n.big = big != 0;
  n.blob_floats = 0;
  const int exp = n.bottleneck ? 4 : 1;
  const std::string r = "backbone_net.resnet.";
  n.stem = add_conv(n, r + "conv1", 3, 64, 7, 2, 3, false);
  add_bn(n, n.stem, r + "bn1");
  int inpl = 64;
  for (int s = 0; s < 4; ++s) {
    const int planes = 64 << s;
    n.planes[s] = planes;
    n.oc[s] = planes * exp;
    for (int j = 0; j < counts[which][s]; ++j) {
      const std::string b = r + "layer" + std::to_string(s + 1) + "." + std::to_string(j) + ".";
      const int st = (j == 0 && s > 0) ? 2 : 1;
      EncBlock blk{-1, -1, -1, -1};
      if (n.bottleneck) {
        blk.c1 = add_conv(n, b + "conv1", inpl, planes, 1, 1, 0, false);
        add_bn(n, blk.c1, b + "bn1");
        blk.c2 = add_conv(n, b + "conv2", planes, planes, 3, st, 1, false);
        add_bn(n, blk.c2, b + "bn2");
        blk.c3 = add_conv(n, b + "conv3", planes, planes * 4, 1, 1, 0, false);
        add_bn(n, blk.c3, b + "bn3");
      } else {
        blk.c1 = add_conv(n, b + "conv1", inpl, planes, 3, st, 1, false);
        add_bn(n, blk.c1, b + "bn1");
        blk.c2 = add_conv(n, b + "conv2", planes, planes, 3, 1, 1, false);
        add_bn(n, blk.c2, b + "bn2");
      }
      if (j == 0 && (st != 1 || inpl != planes * exp)) {
        blk.ds = add_conv(n, b + "downsample.0", inpl, planes * exp, 1, st, 0, false);
        add_bn(n, blk.ds, b + "downsample.1");
      }
      n.stage[s].push_back(blk);
      inpl = planes * exp;
    }
  }
  const std::string d = "decoder_net.resnet_decoder.";
  const int skip_c[4] = {n.oc[2], n.oc[1], n.oc[0], 64};      // stride16, stride8, stride4, stride2
  n.c0d = -1;
  if (!n.big) {
    static const int red[4] = {256, 128, 64, 32}, dout[4] = {256, 128, 64, 64}, fout[4] = {256, 128, 64, 32};
    if (n.deep) n.c0d = add_convs(n, d + "conv0d", {2048, 512}, 1, 0, true)[0];
    int up_in = n.oc[3];
    for (int i = 0; i < 4; ++i) {
      const std::string lv = std::to_string(i + 1);
      n.rc[i] = red[i]; n.dco[i] = dout[i]; n.fo[i] = fout[i];
      n.cd[i] = add_convs(n, d + "conv" + lv + "d", {skip_c[i], red[i]}, 1, 0, true)[0];
      n.dc[i] = add_deconv(n, d + "deconv" + lv, up_in, dout[i]);
      n.cf[i] = add_convs(n, d + "conv" + lv, {red[i] + dout[i], fout[i]}, 3, 1, true)[0];
      up_in = fout[i];
    }
    for (int h = 0; h < 3; ++h)
      n.head[h] = add_convs(n, d + (h == 0 ? "convOut_hm" : h == 1 ? "convOut_hand_seg" : "convOut_obj_seg"), {32, 32, 1}, 1, 0, false);
  } else {
    static const int dout[4] = {1024, 512, 256, 128};
    int up_in = 2048;
    for (int i = 0; i < 4; ++i) {
      const std::string lv = std::to_string(i + 1);
      n.rc[i] = skip_c[i]; n.dco[i] = dout[i]; n.fo[i] = dout[i];
      n.cd[i] = -1;
      n.dc[i] = add_deconv(n, d + "deconv" + lv, up_in, dout[i]);
      n.cf[i] = add_convs(n, d + "conv" + lv, {skip_c[i] + dout[i], dout[i]}, 3, 1, true)[0];
      up_in = dout[i];
    }
    for (int h = 0; h < 3; ++h)
      n.head[h] = add_convs(n, d + (h == 0 ? "convOut_hm" : h == 1 ? "convOut_hand_seg" : "convOut_obj_seg"), {128, 128, 64, 1}, 1, 0, false);
  }
}

bool depth_ok(int t) { return t == 18 || t == 34 || t == 50 || t == 101 || t == 152; }

// descriptor checks shared by every entry; full = the sizes too (the tensor table needs the architecture only)
int check_desc(const char* who, const hoisdf_encoder_desc* d, bool full) {
  HOISDF_REQUIRE(d, HOISDF_ERR_INVALID, "%s: null descriptor", who);
  HOISDF_REQUIRE(depth_ok(d->resnet_type), HOISDF_ERR_INVALID, "%s: resnet_type=%d (18, 34, 50, 101 or 152)", who, d->resnet_type);
  HOISDF_REQUIRE(!d->big_decoder || d->resnet_type >= 50, HOISDF_ERR_INVALID, "%s: big_decoder needs resnet_type >= 50 (got %d)", who,
                 d->resnet_type);
  if (!full) return HOISDF_OK;
  HOISDF_REQUIRE(d->B > 0, HOISDF_ERR_INVALID, "%s: B=%d", who, d->B);
  HOISDF_REQUIRE(d->img_h > 0 && d->img_w > 0 && d->img_h % 32 == 0 && d->img_w % 32 == 0, HOISDF_ERR_INVALID,
                 "%s: image %dx%d: both sides must be positive multiples of 32", who, d->img_h, d->img_w);
  HOISDF_REQUIRE((long)d->B * d->img_h * d->img_w < (1L << 28), HOISDF_ERR_INVALID, "%s: B=%d image %dx%d is too large", who, d->B, d->img_h,
                 d->img_w);
  return HOISDF_OK;
}

const EncNet& net_of(const hoisdf_encoder_desc* d) {
  static thread_local std::map<int, EncNet> cache;
  const int key = d->resnet_type * 2 + (d->big_decoder ? 1 : 0);
  auto it = cache.find(key);
  if (it == cache.end()) {
    it = cache.emplace(key, EncNet{}).first;
    build_net(d->resnet_type, d->big_decoder, it->second);
  }
  return it->second;
}

struct View {
  float* p;
  int ld, C, H, W;
};

// Carves the workspace and (unless dry) enqueues.  A dry run touches no pointer: it answers the activation bytes and the largest
// split-K partial area, which the real run places behind the activations.
struct Exec {
  const hoisdf_encoder_desc* d;
  const EncNet* n;
  const float* blob;
  char* ws;
  bool dry;
  hipStream_t st;
  long off = 0, part_need = 0, part_off = 0, part_bytes = 0;
  int launches = 0;

  float* carve(long floats) {
    float* p = dry ? nullptr : reinterpret_cast<float*>(ws + off);
    off += (floats * (long)sizeof(float) + 255) & ~255L;
    return p;
  }
  View map(int C, int H, int W) { return View{carve((long)d->B * H * W * C), C, C, H, W}; }
  static View slice(const View& v, int c0, int C) { return View{v.p ? v.p + c0 : nullptr, v.ld, C, v.H, v.W}; }

  // out: the destination (slice) with its full geometry; returns the status
  int conv(int id, const View& in, const View& out, int act, const View* res = nullptr) {
    const EncLayer& l = n->layers[id];
    ConvProblem c{d->B, in.H, in.W, l.cin, l.cout, l.k, l.k, l.stride, l.pad, act, l.transposed};
    const int OH = l.transposed ? 2 * in.H : (in.H + 2 * l.pad - l.k) / l.stride + 1;
    const int OW = l.transposed ? 2 * in.W : (in.W + 2 * l.pad - l.k) / l.stride + 1;
    HOISDF_REQUIRE(in.C == l.cin && out.C == l.cout && out.H == OH && out.W == OW, HOISDF_ERR_INVALID,
                   "encoder_infer: layer %d wiring (%d ch %dx%d -> %d ch %dx%d)", id, in.C, in.H, in.W, out.C, out.H, out.W);
    const long M = l.transposed ? (long)d->B * in.H * in.W : (long)d->B * OH * OW;
    const int K = l.transposed ? 4 * l.cin : l.k * l.k * l.cin;
    const ConvPlan p = conv_plan(M, l.cout, K, l.transposed ? 4 : 1);
    if (p.workspace_bytes > part_need) part_need = p.workspace_bytes;
    launches += p.splitk > 1 ? 2 : 1;
    if (dry) return HOISDF_OK;
    return conv_launch(c, in.p, in.ld, blob + l.w_off, blob + l.b_off, res ? res->p : nullptr, res ? res->ld : 0, out.p, out.ld, 0,
                       ws + part_off, part_bytes, st);
  }

  int stage(int s, View in, const View& final_out) {
    const std::vector<EncBlock>& blocks = n->stage[s];
    const int planes = n->planes[s], oc = n->oc[s];
    const int OH = final_out.H, OW = final_out.W;
    View pp[2] = {map(oc, OH, OW), map(oc, OH, OW)};
    View t1 = map(planes, n->bottleneck ? in.H : OH, n->bottleneck ? in.W : OW);
    View t2 = map(planes, OH, OW);
    View dsb = map(oc, OH, OW);
    for (size_t j = 0; j < blocks.size(); ++j) {
      const EncBlock& b = blocks[j];
      const View out = (j + 1 == blocks.size()) ? final_out : pp[j & 1];
      View idt = in;
      if (b.ds >= 0) {
        if (int rc = conv(b.ds, in, dsb, 0)) return rc;
        idt = dsb;
      }
      if (n->bottleneck) {
        View a = t1;
        a.H = in.H; a.W = in.W;                      // conv1 is 1x1 s1: the first block's runs at the stage's input resolution
        if (int rc = conv(b.c1, in, a, 1)) return rc;
        if (int rc = conv(b.c2, a, t2, 1)) return rc;
        if (int rc = conv(b.c3, t2, out, 1, &idt)) return rc;
      } else {
        View a = t1;
        if (int rc = conv(b.c1, in, a, 1)) return rc;
        if (int rc = conv(b.c2, a, out, 1, &idt)) return rc;
      }
      in = out;
    }
    return HOISDF_OK;
  }

  int run(const float* img, float* const* level_out, float* aux_out) {
    const int B = d->B, H = d->img_h, W = d->img_w;
    const int h[5] = {H / 2, H / 4, H / 8, H / 16, H / 32}, w[5] = {W / 2, W / 4, W / 8, W / 16, W / 32};
    auto level = [&](int i, int C) { return View{dry ? nullptr : level_out[i], C, C, h[i], w[i]}; };
    // the concatenated maps of the decoder, level i = 1 .. 4 at stride 16, 8, 4, 2: [reduced (or raw) skip | transposed conv]
    View cat[4];
    for (int i = 0; i < 4; ++i) cat[i] = map(n->rc[i] + n->dco[i], h[3 - i], w[3 - i]);
    // where the backbone's taps go: without a 1x1 reduction the producer writes its slice of the concatenated map itself
    View skip[4];      // stride16, stride8, stride4, stride2
    for (int i = 0; i < 4; ++i) skip[i] = n->cd[i] < 0 ? slice(cat[i], 0, n->rc[i]) : map(i == 3 ? 64 : n->oc[2 - i], h[3 - i], w[3 - i]);
    View top = (n->c0d >= 0) ? map(n->oc[3], h[4], w[4]) : level(4, n->oc[3]);

    const View image{const_cast<float*>(img), 3, 3, H, W};
    if (int rc = conv(n->stem, image, skip[3], 1)) return rc;
    View pooled = map(64, h[1], w[1]);
    ++launches;
    if (!dry)
      if (int rc = maxpool_launch(skip[3].p, skip[3].ld, pooled.p, pooled.ld, B, h[0], w[0], 64, st)) return rc;
    if (int rc = stage(0, pooled, skip[2])) return rc;
    if (int rc = stage(1, skip[2], skip[1])) return rc;
    if (int rc = stage(2, skip[1], skip[0])) return rc;
    if (int rc = stage(3, skip[0], top)) return rc;
    if (n->c0d >= 0)
      if (int rc = conv(n->c0d, top, level(4, 512), 1)) return rc;
    View x = top;                                       // deconv1 reads the stride-32 backbone map, not conv0d's output
    for (int i = 0; i < 4; ++i) {
      if (n->cd[i] >= 0)
        if (int rc = conv(n->cd[i], skip[i], slice(cat[i], 0, n->rc[i]), 1)) return rc;
      if (int rc = conv(n->dc[i], x, slice(cat[i], n->rc[i], n->dco[i]), 1)) return rc;
      const View fused = level(3 - i, n->fo[i]);
      if (int rc = conv(n->cf[i], cat[i], fused, 1)) return rc;
      x = fused;
    }
    if (dry || aux_out) {                               // (a dry run sizes for the call with the aux maps)
      const int hidden = n->layers[n->head[0][0]].cout;
      View hb[2] = {map(hidden, h[0], w[0]), map(hidden, h[0], w[0])};
      const View aux{dry ? nullptr : aux_out, 3, 3, h[0], w[0]};
      for (int k = 0; k < 3; ++k) {
        View cur = x;
        for (size_t li = 0; li < n->head[k].size(); ++li) {
          const int id = n->head[k][li];
          const bool last = li + 1 == n->head[k].size();
          View o = last ? slice(aux, k, 1) : hb[li & 1];
          o.C = n->layers[id].cout;
          if (int rc = conv(id, cur, o, last ? (k == 0 ? 0 : 2) : 1)) return rc;
          cur = o;
        }
      }
    }
    return HOISDF_OK;
  }
};

// activation bytes / partial bytes of the descriptor (dry run)
int size_workspace(const hoisdf_encoder_desc* d, long& act_bytes, long& part_bytes, int* launches = nullptr) {
  Exec e{d, &net_of(d), nullptr, nullptr, true, nullptr};
  if (int rc = e.run(nullptr, nullptr, nullptr)) return rc;
  act_bytes = e.off;
  part_bytes = (e.part_need + 255) & ~255L;
  if (launches) *launches = e.launches;
  return HOISDF_OK;
}

}  // namespace
}  // namespace hoisdf

using namespace hoisdf;

extern "C" int hoisdf_encoder_tensor_count(const hoisdf_encoder_desc* desc) {
  if (check_desc("encoder_tensor_count", desc, false)) return -1;
  return (int)net_of(desc).tensors.size();
}

extern "C" const char* hoisdf_encoder_tensor_name(const hoisdf_encoder_desc* desc, int i) {
  if (check_desc("encoder_tensor_name", desc, false)) return nullptr;
  const EncNet& n = net_of(desc);
  if (i < 0 || i >= (int)n.tensors.size()) {
    set_error("encoder_tensor_name: index %d of %d", i, (int)n.tensors.size());
    return nullptr;
  }
  return n.tensors[i].name.c_str();
}

extern "C" long hoisdf_encoder_tensor_numel(const hoisdf_encoder_desc* desc, int i) {
  if (check_desc("encoder_tensor_numel", desc, false)) return -1;
  const EncNet& n = net_of(desc);
  if (i < 0 || i >= (int)n.tensors.size()) {
    set_error("encoder_tensor_numel: index %d of %d", i, (int)n.tensors.size());
    return -1;
  }
  return n.tensors[i].numel;
}

extern "C" long hoisdf_encoder_prepared_bytes(const hoisdf_encoder_desc* desc) {
  if (check_desc("encoder_prepared_bytes", desc, false)) return -1;
  return net_of(desc).blob_floats * (long)sizeof(float);
}

extern "C" int hoisdf_encoder_prepare(const hoisdf_encoder_desc* desc, const float* const* tensors, int n_tensors, void* prepared,
                                      long prepared_bytes, void* stream) {
  if (int rc = check_desc("encoder_prepare", desc, false)) return rc;
  const EncNet& n = net_of(desc);
  HOISDF_REQUIRE(tensors && prepared, HOISDF_ERR_INVALID, "encoder_prepare: null pointer");
  HOISDF_REQUIRE(n_tensors == (int)n.tensors.size(), HOISDF_ERR_INVALID, "encoder_prepare: %d tensors, the table has %d", n_tensors,
                 (int)n.tensors.size());
  const long need = n.blob_floats * (long)sizeof(float);
  HOISDF_REQUIRE(prepared_bytes >= need, HOISDF_ERR_INVALID, "encoder_prepare: blob of %ld bytes, need %ld", prepared_bytes, need);
  HOISDF_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, HOISDF_ERR_INVALID, "encoder_prepare: the blob must be 256-byte aligned");
  for (int i = 0; i < n_tensors; ++i)
    HOISDF_REQUIRE(tensors[i], HOISDF_ERR_INVALID, "encoder_prepare: null pointer for tensor %d (%s)", i, n.tensors[i].name.c_str());
  float* blob = reinterpret_cast<float*>(prepared);
  for (const EncLayer& l : n.layers) {
    const float* bn = l.t_bn >= 0 ? tensors[l.t_bn] : nullptr;
    if (int rc = conv_pack_launch(tensors[l.t_w], l.t_b >= 0 ? tensors[l.t_b] : nullptr, bn, bn ? tensors[l.t_bn + 1] : nullptr,
                                  bn ? tensors[l.t_bn + 2] : nullptr, bn ? tensors[l.t_bn + 3] : nullptr, BN_EPS, l.cout, l.cin, l.k, l.k,
                                  l.transposed, blob + l.w_off, blob + l.b_off, as_stream(stream)))
      return rc;
  }
  return HOISDF_OK;
}

extern "C" long hoisdf_encoder_infer_workspace(const hoisdf_encoder_desc* desc) {
  if (check_desc("encoder_infer_workspace", desc, true)) return -1;
  long act = 0, part = 0;
  if (size_workspace(desc, act, part)) return -1;
  return act + part;
}

extern "C" int hoisdf_encoder_launch_count(const hoisdf_encoder_desc* desc) {
  if (check_desc("encoder_launch_count", desc, true)) return -1;
  long act = 0, part = 0;
  int launches = 0;
  if (size_workspace(desc, act, part, &launches)) return -1;
  return launches;
}

extern "C" int hoisdf_encoder_pyramid_shape(const hoisdf_encoder_desc* desc, hoisdf_pyramid* shape_only) {
  if (int rc = check_desc("encoder_pyramid_shape", desc, true)) return rc;
  HOISDF_REQUIRE(shape_only, HOISDF_ERR_INVALID, "encoder_pyramid_shape: null pointer");
  const EncNet& n = net_of(desc);
  hoisdf_pyramid& p = *shape_only;
  p.n_levels = 5;
  p.B = desc->B;
  for (int i = 0; i < HOISDF_MAX_LEVELS; ++i) { p.data[i] = nullptr; p.C[i] = p.H[i] = p.W[i] = 0; }
  for (int i = 0; i < 5; ++i) {
    p.H[i] = desc->img_h >> (i + 1);
    p.W[i] = desc->img_w >> (i + 1);
    p.C[i] = i < 4 ? n.fo[3 - i] : (n.c0d >= 0 ? 512 : n.oc[3]);
  }
  return HOISDF_OK;
}

extern "C" int hoisdf_encoder_infer(const hoisdf_encoder_desc* desc, const void* prepared, const float* img_nhwc, float* const* level_out,
                                    float* aux_out, void* workspace, long workspace_bytes, void* stream) {
  if (int rc = check_desc("encoder_infer", desc, true)) return rc;
  HOISDF_REQUIRE(prepared && img_nhwc && level_out && workspace, HOISDF_ERR_INVALID, "encoder_infer: null pointer");
  for (int i = 0; i < 5; ++i) HOISDF_REQUIRE(level_out[i], HOISDF_ERR_INVALID, "encoder_infer: null pointer for level %d", i);
  long act = 0, part = 0;
  if (int rc = size_workspace(desc, act, part)) return rc;
  HOISDF_REQUIRE(workspace_bytes >= act + part, HOISDF_ERR_INVALID, "encoder_infer: workspace of %ld bytes, need %ld", workspace_bytes,
                 act + part);
  HOISDF_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 255) == 0, HOISDF_ERR_INVALID,
                 "encoder_infer: prepared / workspace must be 256-byte aligned");
  Exec e{desc, &net_of(desc), reinterpret_cast<const float*>(prepared), reinterpret_cast<char*>(workspace), false, as_stream(stream)};
  e.part_off = act;
  e.part_bytes = part;
  return e.run(img_nhwc, level_out, aux_out);
}
