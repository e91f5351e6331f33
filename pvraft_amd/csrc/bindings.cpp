// Python bindings for the pvraft_amd CDNA4 kernels (torch extension).
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <utility>

void launch_knn_graph(const float*, int*, int, int, int, hipStream_t);
void launch_knn_csr(const int*, int*, int*, int*, int*, int*, unsigned char*,
                    int, int, int, hipStream_t);
void launch_knn_interp(const float*, const float*, const float*, float*, int*,
                       float*, int, int, int, int, int, float, hipStream_t);
int knn_interp_tile_pts();
void launch_chamfer_fwd(const float*, const float*, const float*, float*, int*,
                        float*, int*, float*, int, int, int, int, int,
                        hipStream_t);
void launch_chamfer_bwd(const float*, const float*, const float*, const int*,
                        const int*, const float*, float*, int, int, int, int,
                        hipStream_t);
int chamfer_fwd_blocks(int, int, int);
int chamfer_tile_pts();
void launch_flow_smooth_fwd(const float*, const int*, float*, int, int, int,
                            int, hipStream_t);
void launch_flow_smooth_bwd(const float*, const int*, const int*, const int*,
                            const float*, float*, int, int, int, int,
                            hipStream_t);
int flow_smooth_blocks(int);
void launch_rigid_fit(const float*, const float*, const float*, float*, float*,
                      float*, unsigned char*, int, int, float, int,
                      hipStream_t);
int rigid_fit_reg_points();
void launch_segmented_rigid_fit(const float*, const float*, const float*,
                                const int*, float*, float*, float*,
                                unsigned char*, int, int, int, float, int,
                                hipStream_t);
int segmented_fit_capacity();
void launch_plane_hypotheses(const float*, const unsigned char*, int*, float*,
                             int*, int, int, int, unsigned, float, float, float,
                             float, float, hipStream_t);
void launch_plane_refine(const float*, const unsigned char*, const float*,
                         const int*, float*, float*, float*, unsigned char*,
                         unsigned char*, int*, int*, int*, unsigned char*,
                         double*, int, int, int, int, double, float, float,
                         float, float, hipStream_t);
int plane_score_tile();
int plane_score_block();
int plane_refine_block();
void launch_cluster_points(const float*, const float*, const unsigned char*,
                           int*, int*, int*, int*, int*, int, int, int, float,
                           float, int, hipStream_t);
int cluster_tile();
void launch_voxel_sample(const float*, const unsigned char*, unsigned long long*,
                         unsigned long long*, int*, unsigned char*, int*, int*,
                         long*, int*, int*, int*, int, int, int, long, int,
                         float, unsigned, hipStream_t);
int voxel_sample_block();
int voxel_sample_scan();
long voxel_sample_meta();
void launch_noise_filter(const float*, const unsigned char*, unsigned long long*,
                         int*, int*, float*, int*, int*, double*, unsigned char*,
                         int*, float*, double*, unsigned char*, int, int, int,
                         float, float, int, int, double, hipStream_t);
int noise_filter_block();
int noise_filter_scan();
void launch_grid_nn_build(const float*, const unsigned char*, unsigned long long*,
                          int*, int*, float*, int*, int*, long, unsigned char*,
                          float*, float*, const float*, const float*, int, int,
                          int, float, hipStream_t);
void launch_grid_nn_query(const float*, const unsigned char*, const float*,
                          const float*, const unsigned long long*, const int*,
                          const float*, const int*, const int*, unsigned char*,
                          int*, float*, float*, float*, int*, int, int, int, int,
                          float, float, float, hipStream_t);
void launch_icp_commit(const int*, const unsigned char*, const float*,
                       const float*, float*, float*, int*, int*, unsigned char*,
                       int, hipStream_t);
int grid_nn_block();
void launch_morton_keys(const float*, const float*, const float*, long*,
                        int, long, hipStream_t);
void launch_gather_edge_fwd(const void*, const int*, const float*, void*,
                            int, int, int, int, bool, hipStream_t);
void launch_gather_edge_bwd(const void*, const int*, float*, int, int, int,
                            int, bool, hipStream_t);
void launch_gather_edge_bwd_csr(const void*, const int*, const int*, void*,
                                int, int, int, int, bool, hipStream_t);
void launch_voxel_corr_fwd(const float*, const float*, const float*, float*,
                           int, int, int, int, float, hipStream_t);
void launch_voxel_corr_bwd(const float*, const float*, const float*, float*,
                           int, int, int, int, float, hipStream_t);
void launch_knn_corr_fwd(const float*, const float*, const float*, float*,
                         int*, int, int, int, int, hipStream_t);
void launch_knn_corr_bwd(const float*, const int*, float*, int, int, int, int,
                         hipStream_t);

void launch_gn_fwd(const void*, void*, float*, float*, float*, const float*,
                   const float*, int, long, long, int, int, float, int, float,
                   const float*, bool, hipStream_t);
void launch_gn_bwd(const void*, const void*, const float*, const float*,
                   const float*, const float*, float*, float*, float*,
                   float*, int, void*, int, long, long, int, int, int, float,
                   const float*, bool, hipStream_t);
int gn_reduce_chunks(long, int, int, int);
int gnmp_reduce_chunks(long, int, int, int, int);
int gnmp_bwd_reduce_chunks(long, int, int, int);
void launch_gnmp_fwd(const void*, void*, unsigned char*, float*, float*,
                     float*, const float*, const float*, int, long, long, int,
                     int, int, float, int, float, const float*, bool,
                     hipStream_t);
void launch_pv_corr_fused_fwd(const float*, const float*, const float*,
                              float*, float*, int*, int, int, int, int, int,
                              float, hipStream_t);
void launch_pv_corr_fused_bwd(const float*, const float*, const float*,
                              const float*, const int*, float*, int, int, int,
                              int, int, float, hipStream_t);
void launch_topk_rows(const float*, float*, int*, long, int, int,
                      hipStream_t);
void launch_seq_loss_fwd(const float* const*, const float*, const float*,
                         float*, float*, float*, long, int, int, float,
                         hipStream_t);
void launch_seq_loss_bwd(const float* const*, float* const*, const float*,
                         const float*, const float*, const float*, long, int,
                         int, float, hipStream_t);
void launch_gru_zr_fwd(const void*, const void*, void*, void*, void*, long,
                       long, bool, hipStream_t);
void launch_gru_zr_bwd(const void*, const void*, const void*, const void*,
                       const void*, void*, void*, long, long, bool,
                       hipStream_t);
void launch_gru_q_fwd(const void*, const void*, const void*, void*, void*,
                      long, long, bool, hipStream_t);
void launch_gru_q_bwd(const void*, const void*, const void*, const void*,
                      void*, void*, void*, long, long, bool, hipStream_t);
void launch_transpose(const void*, void*, long, int, long, long, bool,
                      hipStream_t);
void launch_pw_wgrad(const void*, const void*, float*, float*, int, int, int,
                     long, int, hipStream_t);
void launch_gn_bwd_extract(float*, float*, float*, float*, int, int, int,
                           hipStream_t);
void launch_egnmp_fwd(const void*, const int*, float*, float*, float*,
                      float*, const float*, const float*, float*, float*,
                      unsigned char*, unsigned char*, float*, void*,
                      unsigned char*, float*,
                      int, long, int, int, int, float, int, float,
                      const float*, bool, int, bool, bool, hipStream_t);
void launch_egnmp_bwd(const void*, const void*, const int*,
                      const unsigned char*, const float*, const float*,
                      const int*, const int*,
                      const unsigned char*, const float*, const float*,
                      const float*, const float*, float*, float*, float*,
                      void*, int, long, int, int, int, int, float,
                      const float*, bool, int, bool, hipStream_t);
int egnmp_reduce_chunks(long, int, int);
struct CastDesc { const float* src; void* dst; int n; };
struct CastChunk { CastDesc d[128]; int count; };
void launch_multi_cast(const CastChunk*, int, hipStream_t);
void launch_kg_fwd(const float*, const float*, const float*, float*, float*,
                   float*, float*, const float*, const float*, float*,
                   float*, unsigned char*, unsigned char*, void*,
                   unsigned char*, float*, int, long, int, int, int, float,
                   const float*, bool, int, bool, hipStream_t);
void launch_kg_bwd(const void*, bool, const float*, const float*,
                   const float*, const unsigned char*, const float*,
                   const float*, const float*, const float*, const float*,
                   float*, float*, double*, float*, unsigned char*, float*,
                   float*, float*, float*, float*, float*, bool, int, long,
                   int, int, int, float, const float*, bool, hipStream_t);
long kg_bwd_part_len(int, long, int, int);
long kg_bwd_pgrad_len(int, int);
void launch_gnmp_bwd(const void*, const void*, const unsigned char*,
                     const float*, const float*, const float*, const float*,
                     float*, float*, float*, float*, int, void*, int, long,
                     long, int, int, int, int, float, const float*, bool,
                     hipStream_t);

namespace {

void check_f32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must be float32");
}

hipStream_t stream() { return at::hip::getCurrentHIPStream().stream(); }

// zero-filled workspace via hipMemsetAsync (cheaper than an ATen fill
// kernel; these workspaces are allocated on every call and the fill
// launches were ~2 ms/step in aggregate).
//
// NEVER memset while the stream is capturing into a hipGraph: on ROCm 7.2
// a memset enqueued during capture is mis-ordered at replay against the
// kernels consuming the workspace -- replays then intermittently read
// partially-zeroed GroupNorm/wgrad workspaces and produce garbage
// gradients (reproduced 6/6 at tiny config, OK 6/6 with the memset
// disabled; see profiles/README.md).  Inside capture the plain fill
// kernel is captured instead, which replays correctly.
torch::Tensor zeros_fast(at::IntArrayRef sizes,
                         const torch::TensorOptions& opt) {
  static const bool disabled = [] {
    const char* e = getenv("PVRAFT_NO_MEMSET");
    return e && e[0] == '1';
  }();
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  hipStreamIsCapturing(stream(), &cap);
  if (disabled || cap != hipStreamCaptureStatusNone)
    return torch::zeros(sizes, opt);
  auto t = torch::empty(sizes, opt);
  if (t.numel() > 0)
    hipMemsetAsync(t.data_ptr(), 0, t.numel() * t.element_size(), stream());
  return t;
}

// persistent zero workspace for the GN forward reduction: the finalize
// kernel re-zeroes it after consuming, so one buffer per size serves every
// call and every hipGraph replay (stream-ordered) with no per-call
// allocation or fill.  Held forever (a few KB total).
torch::Tensor& persistent_ws(long len, const torch::TensorOptions& opt) {
  // leaked on purpose: a static map of CUDA tensors must not run its
  // destructor during process teardown (races CUDA context destruction)
  static auto* cache = new std::unordered_map<long, torch::Tensor>();
  auto it = cache->find(len);
  if (it == cache->end())
    it = cache->emplace(len, torch::zeros({len}, opt)).first;
  return it->second;
}

// persistent_ws is keyed by length alone, so two workspaces of equal
// length are the same tensor.  An op that holds several workspaces at once
// names each one's role; a role's buffers never alias another role's or a
// plain persistent_ws buffer.  Contents are unspecified between calls.
torch::Tensor& persistent_ws_role(const char* role, long len,
                                  const torch::TensorOptions& opt) {
  static auto* cache =
      new std::map<std::pair<std::string, long>, torch::Tensor>();
  const auto key = std::make_pair(std::string(role), len);
  auto it = cache->find(key);
  if (it == cache->end())
    it = cache->emplace(key, torch::zeros({len}, opt)).first;
  return it->second;
}

}  // namespace

torch::Tensor morton_keys(torch::Tensor xyz, torch::Tensor mn,
                          torch::Tensor inv_ext) {
  check_f32(xyz, "xyz");
  check_f32(mn, "mn");
  check_f32(inv_ext, "inv_ext");
  TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "xyz must be (B,N,3)");
  const int B = xyz.size(0);
  const long N = xyz.size(1);
  auto keys = torch::empty({B, N}, xyz.options().dtype(torch::kInt64));
  launch_morton_keys(xyz.data_ptr<float>(), mn.data_ptr<float>(),
                     inv_ext.data_ptr<float>(), keys.data_ptr<long>(), B, N,
                     stream());
  return keys;
}

torch::Tensor knn_graph(torch::Tensor xyz, int64_t k) {
  check_f32(xyz, "xyz");
  TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "xyz must be (B,N,3)");
  const int B = xyz.size(0), N = xyz.size(1);
  TORCH_CHECK(k >= 1 && k <= 48 && k <= N, "knn_graph requires 1 <= k <= 48, k <= N");
  auto out = torch::empty({B, N, k}, xyz.options().dtype(torch::kInt32));
  launch_knn_graph(xyz.data_ptr<float>(), out.data_ptr<int>(), B, N, (int)k,
                   stream());
  return out;
}

// idx32 (B,N,k) int32 contiguous -> {order (B,k*N) i32, offsets (B,N+1) i32,
// order_n (B,k*N) i32, order_j (B,k*N) u8}: edge ids j*N+n sorted by
// (target, id) -- the inverse adjacency of the kNN graph (csrc/knn_csr.hip)
std::vector<torch::Tensor> knn_csr(torch::Tensor idx32) {
  TORCH_CHECK(idx32.is_cuda() && idx32.is_contiguous() && idx32.dim() == 3 &&
              idx32.scalar_type() == torch::kInt32,
              "idx32 must be a contiguous (B,N,k) int32 GPU tensor");
  const int64_t B = idx32.size(0), N = idx32.size(1), k = idx32.size(2);
  TORCH_CHECK(k >= 1 && k <= 48, "knn_csr requires 1 <= k <= 48");
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1 && k * N < (1L << 31) - 256,
              "knn_csr requires 1 <= B <= 65535, N >= 1, k*N < 2^31");
  auto iopt = idx32.options();
  auto order = torch::empty({B, k * N}, iopt);
  auto offsets = torch::empty({B, N + 1}, iopt);
  auto order_n = torch::empty({B, k * N}, iopt);
  auto order_j = torch::empty({B, k * N}, iopt.dtype(torch::kUInt8));
  auto bucket = torch::empty({B, k * N}, iopt);
  auto cnt = zeros_fast({B, N}, iopt);
  launch_knn_csr(idx32.data_ptr<int>(), cnt.data_ptr<int>(),
                 bucket.data_ptr<int>(), order.data_ptr<int>(),
                 offsets.data_ptr<int>(), order_n.data_ptr<int>(),
                 order_j.data_ptr<unsigned char>(), (int)B, (int)N, (int)k,
                 stream());
  return {order, offsets, order_n, order_j};
}

// support (B,N,3), values (B,N,C), query (B,M,3), all fp32 contiguous ->
// {out (B,M,C) f32, idx (B,M,min(k,N)) i32, w (B,M,min(k,N)) f32}
std::vector<torch::Tensor> knn_interp_fwd(torch::Tensor support,
                                          torch::Tensor values,
                                          torch::Tensor query, int64_t k,
                                          double eps) {
  check_f32(support, "support_xyz");
  check_f32(values, "values");
  check_f32(query, "query_xyz");
  TORCH_CHECK(support.dim() == 3 && support.size(2) == 3, "support_xyz must be (B,N,3)");
  TORCH_CHECK(query.dim() == 3 && query.size(2) == 3, "query_xyz must be (B,M,3)");
  TORCH_CHECK(values.dim() == 3, "values must be (B,N,C)");
  TORCH_CHECK(values.device() == support.device() && query.device() == support.device(),
              "knn_interp inputs must share a device");
  const int64_t B = support.size(0), N = support.size(1);
  const int64_t M = query.size(1), C = values.size(2);
  TORCH_CHECK(query.size(0) == B && values.size(0) == B && values.size(1) == N,
              "knn_interp batch / support size mismatch");
  TORCH_CHECK(k >= 1 && k <= 16, "knn_interp requires 1 <= k <= 16");
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1 && M >= 1 && C >= 1,
              "knn_interp requires 1 <= B <= 65535, N, M, C >= 1");
  TORCH_CHECK(N < (1L << 31) / 4 && M < (1L << 31) - 256 && C < (1L << 31),
              "knn_interp sizes exceed 32-bit point indexing");
  TORCH_CHECK(eps >= 0.0, "knn_interp requires eps >= 0");
  const int keff = (int)std::min<int64_t>(k, N);
  auto out = torch::empty({B, M, C}, values.options());
  auto idx = torch::empty({B, M, keff}, values.options().dtype(torch::kInt32));
  auto w = torch::empty({B, M, keff}, values.options());
  launch_knn_interp(support.data_ptr<float>(), values.data_ptr<float>(),
                    query.data_ptr<float>(), out.data_ptr<float>(),
                    idx.data_ptr<int>(), w.data_ptr<float>(), (int)B, (int)N,
                    (int)M, (int)C, keff, (float)eps, stream());
  return {out, idx, w};
}

torch::Tensor gather_edge_concat_fwd(torch::Tensor feats, torch::Tensor idx,
                                     torch::Tensor xyz) {
  TORCH_CHECK(feats.is_cuda() && feats.is_contiguous(), "feats must be contiguous GPU");
  check_f32(xyz, "xyz");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.is_contiguous(), "idx must be contiguous int32");
  const bool bf16 = feats.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || feats.scalar_type() == torch::kFloat32, "fp32/bf16 only");
  const int B = feats.size(0), N = feats.size(1), C = feats.size(2), K = idx.size(2);
  auto out = torch::empty({B, C + 3, K, N}, feats.options());
  launch_gather_edge_fwd(feats.data_ptr(), idx.data_ptr<int>(),
                         xyz.data_ptr<float>(), out.data_ptr(), B, N, K, C,
                         bf16, stream());
  return out;
}

torch::Tensor gather_edge_concat_bwd(torch::Tensor gout, torch::Tensor idx,
                                     int64_t C) {
  TORCH_CHECK(gout.is_cuda() && gout.is_contiguous(), "gout must be contiguous GPU");
  const bool bf16 = gout.scalar_type() == torch::kBFloat16;
  const int B = gout.size(0), K = gout.size(2), N = gout.size(3);
  TORCH_CHECK(gout.size(1) == C + 3, "gout channel mismatch");
  auto gfeats = torch::empty({B, N, C}, gout.options().dtype(torch::kFloat32));
  launch_gather_edge_bwd(gout.data_ptr(), idx.data_ptr<int>(),
                         gfeats.data_ptr<float>(), B, N, K, (int)C, bf16,
                         stream());
  return bf16 ? gfeats.to(torch::kBFloat16) : gfeats;
}

torch::Tensor gather_edge_bwd_csr(torch::Tensor gT, torch::Tensor order,
                                  torch::Tensor offsets, int64_t K) {
  TORCH_CHECK(gT.is_cuda() && gT.is_contiguous(), "gT must be contiguous GPU");
  const bool bf16 = gT.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || gT.scalar_type() == torch::kFloat32, "fp32/bf16 only");
  TORCH_CHECK(order.scalar_type() == torch::kInt32 && order.is_contiguous());
  TORCH_CHECK(offsets.scalar_type() == torch::kInt32 && offsets.is_contiguous());
  const int B = gT.size(0), NK = gT.size(1), C = gT.size(2);
  const int N = NK / (int)K;
  auto grad = torch::empty({B, N, C}, gT.options());
  launch_gather_edge_bwd_csr(gT.data_ptr(), order.data_ptr<int>(),
                             offsets.data_ptr<int>(), grad.data_ptr(), B, N,
                             (int)K, C, bf16, stream());
  return grad;
}

torch::Tensor voxel_corr_fwd(torch::Tensor corr, torch::Tensor xyz,
                             torch::Tensor coords, double base_scale,
                             int64_t num_levels, int64_t resolution) {
  check_f32(corr, "corr");
  check_f32(xyz, "xyz");
  check_f32(coords, "coords");
  TORCH_CHECK(resolution == 3, "HIP voxel_corr supports resolution=3");
  TORCH_CHECK(num_levels >= 1 && num_levels <= 4, "1 <= num_levels <= 4");
  const int B = corr.size(0), N = corr.size(1), K = corr.size(2);
  auto out = torch::empty({B, num_levels * 27, N}, corr.options());
  launch_voxel_corr_fwd(corr.data_ptr<float>(), xyz.data_ptr<float>(),
                        coords.data_ptr<float>(), out.data_ptr<float>(), B, N,
                        K, (int)num_levels, (float)base_scale, stream());
  return out;
}

torch::Tensor voxel_corr_bwd(torch::Tensor gout, torch::Tensor xyz,
                             torch::Tensor coords, double base_scale,
                             int64_t num_levels, int64_t resolution) {
  check_f32(gout, "gout");
  TORCH_CHECK(resolution == 3, "HIP voxel_corr supports resolution=3");
  const int B = xyz.size(0), N = xyz.size(1), K = xyz.size(2);
  auto gcorr = torch::empty({B, N, K}, gout.options());
  launch_voxel_corr_bwd(gout.data_ptr<float>(), xyz.data_ptr<float>(),
                        coords.data_ptr<float>(), gcorr.data_ptr<float>(), B,
                        N, K, (int)num_levels, (float)base_scale, stream());
  return gcorr;
}

std::vector<torch::Tensor> knn_corr_fwd(torch::Tensor corr, torch::Tensor xyz,
                                        torch::Tensor coords, int64_t k) {
  check_f32(corr, "corr");
  check_f32(xyz, "xyz");
  check_f32(coords, "coords");
  const int B = corr.size(0), N = corr.size(1), K = corr.size(2);
  TORCH_CHECK(K <= 512, "HIP knn_corr supports K <= 512");
  TORCH_CHECK(k >= 1 && k <= K, "need 1 <= k <= K");
  auto out = torch::empty({B, 4, k, N}, corr.options());
  auto idx = torch::empty({B, N, k}, corr.options().dtype(torch::kInt32));
  launch_knn_corr_fwd(corr.data_ptr<float>(), xyz.data_ptr<float>(),
                      coords.data_ptr<float>(), out.data_ptr<float>(),
                      idx.data_ptr<int>(), B, N, K, (int)k, stream());
  return {out, idx};
}

torch::Tensor knn_corr_bwd(torch::Tensor gout, torch::Tensor idx, int64_t K) {
  check_f32(gout, "gout");
  const int B = gout.size(0), k = gout.size(2), N = gout.size(3);
  auto gcorr = zeros_fast({B, N, K}, gout.options());
  launch_knn_corr_bwd(gout.data_ptr<float>(), idx.data_ptr<int>(),
                      gcorr.data_ptr<float>(), B, N, (int)K, k, stream());
  return gcorr;
}

// x (B, C, S) contiguous (S = flattened spatial); weight/bias (C) fp32.
// act: 0 none, 1 LeakyReLU(slope).  Returns {y, mean (B*G), rstd (B*G)}.
// slope_t: scalar fp32 tensor for act==2 (learnable PReLU slope)
std::vector<torch::Tensor> group_norm_act_fwd(torch::Tensor x, int64_t G,
                                              torch::Tensor weight,
                                              torch::Tensor bias, double eps,
                                              int64_t act, double slope,
                                              c10::optional<torch::Tensor> slope_t) {
  const float* slope_ptr = nullptr;
  if (act == 2) {
    TORCH_CHECK(slope_t.has_value() && slope_t->numel() == 1, "act=2 needs a scalar slope tensor");
    slope_ptr = slope_t->data_ptr<float>();
  }
  TORCH_CHECK(x.is_cuda() && x.is_contiguous(), "x must be contiguous GPU");
  TORCH_CHECK(x.dim() == 3, "x must be (B, C, S)");
  check_f32(weight, "weight");
  check_f32(bias, "bias");
  const int B = x.size(0), C = x.size(1);
  const long S = x.size(2);
  TORCH_CHECK(C % G == 0, "C % G != 0");
  const int rows = B * G;
  const long row_len = (C / G) * S;
  auto fopt = x.options().dtype(torch::kFloat32);
  // per-call deterministic partial-sum scratch (one slot pair per reduce
  // block) -- no persistent zeroed workspace, no finalize launch
  const int rchunks = gn_reduce_chunks(S, B, C, (int)G);
  auto scratch = torch::empty({(long)B * C * 2 * rchunks}, fopt);
  auto mean = torch::empty({rows}, fopt);
  auto rstd = torch::empty({rows}, fopt);
  auto y = torch::empty_like(x);
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat32,
              "group_norm_act: dtype must be float32 or bfloat16");
  launch_gn_fwd(x.data_ptr(), y.data_ptr(), scratch.data_ptr<float>(),
                mean.data_ptr<float>(), rstd.data_ptr<float>(),
                weight.data_ptr<float>(), bias.data_ptr<float>(), rows,
                row_len, S, C, (int)G, (float)eps, (int)act, (float)slope,
                slope_ptr, bf16, stream());
  return {y, mean, rstd};
}


// Finish a GN-family backward: either materialise fresh dweight/dbias/
// dslope tensors (plain autograd) or ACCUMULATE into the parameters' own
// fp32 grad buffers (deferred mode, returns an empty vector tail).
static std::vector<torch::Tensor> gn_grads_finish(
    torch::Tensor& ws, torch::Tensor dx, int rows, int C,
    const torch::TensorOptions& fopt,
    c10::optional<torch::Tensor> wt, c10::optional<torch::Tensor> bt,
    c10::optional<torch::Tensor> st) {
  if (wt.has_value()) {
    TORCH_CHECK(wt->is_cuda() && wt->is_contiguous() &&
                wt->scalar_type() == torch::kFloat32 && wt->numel() == C &&
                bt.has_value() && bt->numel() == C,
                "gn accumulate targets must be fp32 (C)");
    float* sp = nullptr;
    if (st.has_value() && st->defined() && st->numel() == 1)
      sp = st->data_ptr<float>();
    launch_gn_bwd_extract(ws.data_ptr<float>(), wt->data_ptr<float>(),
                          bt->data_ptr<float>(), sp, rows, C, 1, stream());
    return {dx};
  }
  auto dweight = torch::empty({C}, fopt);
  auto dbias = torch::empty({C}, fopt);
  auto dslope = torch::empty({1}, fopt);
  launch_gn_bwd_extract(ws.data_ptr<float>(), dweight.data_ptr<float>(),
                        dbias.data_ptr<float>(), dslope.data_ptr<float>(),
                        rows, C, 0, stream());
  return {dx, dweight, dbias, dslope};
}

std::vector<torch::Tensor> group_norm_act_bwd(torch::Tensor dy, torch::Tensor x,
                                              torch::Tensor mean,
                                              torch::Tensor rstd, int64_t G,
                                              torch::Tensor weight,
                                              torch::Tensor bias, int64_t act,
                                              double slope,
                                              c10::optional<torch::Tensor> slope_t,
                                              c10::optional<torch::Tensor> wtarget = c10::nullopt,
                                              c10::optional<torch::Tensor> btarget = c10::nullopt,
                                              c10::optional<torch::Tensor> starget = c10::nullopt) {
  const float* slope_ptr = nullptr;
  if (act == 2) {
    TORCH_CHECK(slope_t.has_value() && slope_t->numel() == 1, "act=2 needs a scalar slope tensor");
    slope_ptr = slope_t->data_ptr<float>();
  }
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(), "dy/x must be contiguous");
  const int B = x.size(0), C = x.size(1);
  const long S = x.size(2);
  const int rows = B * G;
  const long row_len = (C / G) * S;
  auto fopt = x.options().dtype(torch::kFloat32);
  const int rchunks = gn_reduce_chunks(S, B, C, (int)G);
  auto scratch = torch::empty({(long)B * C * 5 * rchunks}, fopt);
  auto dx = torch::empty_like(x);
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat32,
              "group_norm_act: dtype must be float32 or bfloat16");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type(), "dy/x dtype mismatch");
  // channel grads drain inside the apply pass: into fresh tensors, or
  // ACCUMULATED into the parameters' grad buffers (deferred mode)
  torch::Tensor dweight, dbias, dslope;
  float *dwp, *dbp, *dsp;
  int accumulate = 0;
  if (wtarget.has_value()) {
    accumulate = 1;
    dwp = wtarget->data_ptr<float>();
    dbp = btarget->data_ptr<float>();
    dsp = (starget.has_value() && starget->defined() && starget->numel() == 1)
              ? starget->data_ptr<float>() : nullptr;
  } else {
    dweight = torch::empty({C}, fopt);
    dbias = torch::empty({C}, fopt);
    dslope = torch::empty({1}, fopt);
    dwp = dweight.data_ptr<float>();
    dbp = dbias.data_ptr<float>();
    dsp = dslope.data_ptr<float>();
  }
  launch_gn_bwd(dy.data_ptr(), x.data_ptr(), mean.data_ptr<float>(),
                rstd.data_ptr<float>(), weight.data_ptr<float>(),
                bias.data_ptr<float>(), scratch.data_ptr<float>(), dwp, dbp,
                dsp, accumulate, dx.data_ptr(), rows, row_len, S, C, (int)G,
                (int)act, (float)slope, slope_ptr, bf16, stream());
  if (accumulate) return {dx};
  return {dx, dweight, dbias, dslope};
}

// x (B, C, K, N); GN stats over full (K, N); returns pooled
// {y (B,C,N), argmax (B,C,N) u8, mean, rstd}
std::vector<torch::Tensor> group_norm_act_maxpool_fwd(
    torch::Tensor x, int64_t G, torch::Tensor weight, torch::Tensor bias,
    double eps, int64_t act, double slope,
    c10::optional<torch::Tensor> slope_t) {
  const float* slope_ptr = nullptr;
  if (act == 2) {
    TORCH_CHECK(slope_t.has_value() && slope_t->numel() == 1, "act=2 needs a scalar slope tensor");
    slope_ptr = slope_t->data_ptr<float>();
  }
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 4, "x must be contiguous (B,C,K,N)");
  check_f32(weight, "weight");
  check_f32(bias, "bias");
  const int B = x.size(0), C = x.size(1), K = x.size(2);
  const long N = x.size(3);
  TORCH_CHECK(K <= 255, "maxpool K must fit u8 argmax");
  const int rows = B * G;
  const long row_len = (C / G) * K * N;
  auto fopt = x.options().dtype(torch::kFloat32);
  const int rchunks = gnmp_reduce_chunks(N, K, B, C, (int)G);
  auto scratch = torch::empty({(long)B * C * 2 * rchunks}, fopt);
  auto mean = torch::empty({rows}, fopt);
  auto rstd = torch::empty({rows}, fopt);
  auto y = torch::empty({B, C, N}, x.options());
  auto am = torch::empty({B, C, N}, x.options().dtype(torch::kUInt8));
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat32, "fp32/bf16 only");
  launch_gnmp_fwd(x.data_ptr(), y.data_ptr(), am.data_ptr<unsigned char>(),
                  scratch.data_ptr<float>(), mean.data_ptr<float>(),
                  rstd.data_ptr<float>(), weight.data_ptr<float>(),
                  bias.data_ptr<float>(), rows, row_len, N, K, C, (int)G,
                  (float)eps, (int)act, (float)slope, slope_ptr, bf16, stream());
  return {y, am, mean, rstd};
}

std::vector<torch::Tensor> group_norm_act_maxpool_bwd(
    torch::Tensor dy, torch::Tensor x, torch::Tensor am, torch::Tensor mean,
    torch::Tensor rstd, int64_t G, torch::Tensor weight, torch::Tensor bias,
    int64_t act, double slope, c10::optional<torch::Tensor> slope_t,
    c10::optional<torch::Tensor> wtarget = c10::nullopt,
    c10::optional<torch::Tensor> btarget = c10::nullopt,
    c10::optional<torch::Tensor> starget = c10::nullopt) {
  const float* slope_ptr = nullptr;
  if (act == 2) {
    TORCH_CHECK(slope_t.has_value() && slope_t->numel() == 1, "act=2 needs a scalar slope tensor");
    slope_ptr = slope_t->data_ptr<float>();
  }
  TORCH_CHECK(dy.is_contiguous() && x.is_contiguous(), "dy/x must be contiguous");
  const int B = x.size(0), C = x.size(1), K = x.size(2);
  const long N = x.size(3);
  const int rows = B * G;
  const long row_len = (C / G) * K * N;
  auto fopt = x.options().dtype(torch::kFloat32);
  const int rchunks = gnmp_bwd_reduce_chunks(N, B, C, (int)G);
  auto scratch = torch::empty({(long)B * C * 5 * rchunks}, fopt);
  auto dx = torch::empty_like(x);
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  torch::Tensor dweight, dbias, dslope;
  float *dwp, *dbp, *dsp;
  int accumulate = 0;
  if (wtarget.has_value()) {
    accumulate = 1;
    dwp = wtarget->data_ptr<float>();
    dbp = btarget->data_ptr<float>();
    dsp = (starget.has_value() && starget->defined() && starget->numel() == 1)
              ? starget->data_ptr<float>() : nullptr;
  } else {
    dweight = torch::empty({C}, fopt);
    dbias = torch::empty({C}, fopt);
    dslope = torch::empty({1}, fopt);
    dwp = dweight.data_ptr<float>();
    dbp = dbias.data_ptr<float>();
    dsp = dslope.data_ptr<float>();
  }
  launch_gnmp_bwd(dy.data_ptr(), x.data_ptr(), am.data_ptr<unsigned char>(),
                  mean.data_ptr<float>(), rstd.data_ptr<float>(),
                  weight.data_ptr<float>(), bias.data_ptr<float>(),
                  scratch.data_ptr<float>(), dwp, dbp, dsp, accumulate,
                  dx.data_ptr(), rows, row_len, N, K, C, (int)G, (int)act,
                  (float)slope, slope_ptr, bf16, stream());
  if (accumulate) return {dx};
  return {dx, dweight, dbias, dslope};
}

// SetConv stage 1 on the linearly-restructured operands: wg (B, N, M)
// point-major = (fc1 W @ [feats; xyz]) per point; pooled output y and u8
// argmax are point-major too.  GN stats over the full (M/G, K, N) edge
// extent, identical to group_norm_act_maxpool.  channel_major_out: y is
// written (B, M, N) instead (am/vsel stay point-major for the backward).
// classic (here and in edge_gnmp_bwd): run the one-gather-per-iteration
// kernels instead of the batched ones (PVRAFT_EGNMP, for A/B runs).
std::vector<torch::Tensor> edge_gnmp_fwd(torch::Tensor wg, torch::Tensor idx,
                                         int64_t G, torch::Tensor weight,
                                         torch::Tensor bias, double eps,
                                         int64_t act, double slope,
                                         c10::optional<torch::Tensor> slope_t,
                                         bool channel_major_out = false,
                                         bool classic = false) {
  const float* slope_ptr = nullptr;
  if (act == 2) {
    TORCH_CHECK(slope_t.has_value() && slope_t->numel() == 1, "act=2 needs a scalar slope tensor");
    slope_ptr = slope_t->data_ptr<float>();
  }
  TORCH_CHECK(wg.is_cuda() && wg.is_contiguous() && wg.dim() == 3, "wg must be contiguous (B,N,M)");
  TORCH_CHECK(idx.scalar_type() == torch::kInt32 && idx.is_contiguous(), "idx must be contiguous int32");
  check_f32(weight, "weight");
  check_f32(bias, "bias");
  const int B = wg.size(0), M = wg.size(2), K = idx.size(2);
  const long N = wg.size(1);
  TORCH_CHECK(idx.size(0) == B && idx.size(1) == N, "idx/wg shape mismatch");
  TORCH_CHECK(M % G == 0 && G <= 8 && M <= 256 && M % 4 == 0,
              "edge_gnmp: need M % G == 0, M % 4 == 0, G <= 8, M <= 256");
  TORCH_CHECK(K <= 255, "edge_gnmp: K must fit u8 argmax");
  const bool bf16 = wg.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || wg.scalar_type() == torch::kFloat32, "fp32/bf16 only");
  const int rows = B * (int)G;
  auto fopt = wg.options().dtype(torch::kFloat32);
  auto& ws = persistent_ws((long)rows * 2, fopt);
  const int rchunks = egnmp_reduce_chunks(N, M, B);
  auto scratch = torch::empty({(long)rows * 2, (long)rchunks * B}, fopt);
  auto mean = torch::empty({rows}, fopt);
  auto rstd = torch::empty({rows}, fopt);
  auto y = channel_major_out ? torch::empty({B, (long)M, N}, wg.options())
                             : torch::empty_like(wg);
  auto am = torch::empty({B, N, M}, wg.options().dtype(torch::kUInt8));
  // per-(n, c) gather extremes tracked by the reduce pass (the pick pass
  // is elementwise; the second full gather sweep is gone).  fp32: the
  // backward derives activation-branch signs from them.
  auto vmax = torch::empty({B, N, M}, fopt);
  auto vmin = torch::empty({B, N, M}, fopt);
  auto amax = torch::empty({B, N, M}, wg.options().dtype(torch::kUInt8));
  auto amin = torch::empty({B, N, M}, wg.options().dtype(torch::kUInt8));
  // saved for the closed-form backward centre term: per-point gather sum
  // (fp32) and the selected pre-GN extreme value
  auto vsum = torch::empty({B, N, M}, fopt);
  auto vsel = torch::empty({B, N, M}, fopt);
  launch_egnmp_fwd(wg.data_ptr(), idx.data_ptr<int>(),
                   scratch.data_ptr<float>(), ws.data_ptr<float>(),
                   mean.data_ptr<float>(), rstd.data_ptr<float>(),
                   weight.data_ptr<float>(), bias.data_ptr<float>(),
                   vmax.data_ptr<float>(), vmin.data_ptr<float>(),
                   amax.data_ptr<unsigned char>(),
                   amin.data_ptr<unsigned char>(), vsum.data_ptr<float>(),
                   y.data_ptr(),
                   am.data_ptr<unsigned char>(), vsel.data_ptr<float>(), B, N,
                   K, M, (int)G, (float)eps, (int)act, (float)slope,
                   slope_ptr, bf16, rchunks, channel_major_out, classic,
                   stream());
  return {y, am, vsel, vsum, mean, rstd};
}

std::vector<torch::Tensor> edge_gnmp_bwd(
    torch::Tensor dy, torch::Tensor wg, torch::Tensor idx, torch::Tensor am,
    torch::Tensor vsel, torch::Tensor vsum,
    torch::Tensor offsets, torch::Tensor order_n, torch::Tensor order_j,
    torch::Tensor mean, torch::Tensor rstd, int64_t G,
    torch::Tensor weight, torch::Tensor bias,
    int64_t act, double slope, c10::optional<torch::Tensor> slope_t,
    c10::optional<torch::Tensor> wtarget = c10::nullopt,
    c10::optional<torch::Tensor> btarget = c10::nullopt,
    c10::optional<torch::Tensor> starget = c10::nullopt,
    bool classic = false) {
  const float* slope_ptr = nullptr;
  if (act == 2) {
    TORCH_CHECK(slope_t.has_value() && slope_t->numel() == 1, "act=2 needs a scalar slope tensor");
    slope_ptr = slope_t->data_ptr<float>();
  }
  TORCH_CHECK(dy.is_contiguous() && wg.is_contiguous(), "dy/wg must be contiguous");
  TORCH_CHECK(dy.scalar_type() == wg.scalar_type(), "dy/wg dtype mismatch");
  TORCH_CHECK(offsets.scalar_type() == torch::kInt32 && offsets.is_contiguous());
  TORCH_CHECK(order_n.scalar_type() == torch::kInt32 && order_n.is_contiguous());
  TORCH_CHECK(order_j.scalar_type() == torch::kUInt8 && order_j.is_contiguous());
  TORCH_CHECK(offsets.scalar_type() == torch::kInt32 && offsets.is_contiguous());
  TORCH_CHECK(order_n.scalar_type() == torch::kInt32 && order_n.is_contiguous());
  TORCH_CHECK(order_j.scalar_type() == torch::kUInt8 && order_j.is_contiguous());
  const int B = wg.size(0), M = wg.size(2), K = idx.size(2);
  const long N = wg.size(1);
  const bool bf16 = wg.scalar_type() == torch::kBFloat16;
  const int rows = B * (int)G;
  auto fopt = wg.options().dtype(torch::kFloat32);
  const long ws_len = (long)rows * 2 + M * 2 + 1;
  auto& ws = persistent_ws(ws_len, fopt);
  const int rchunks = egnmp_reduce_chunks(N, M, B);
  auto scratch = torch::empty({ws_len, (long)rchunks * B}, fopt);
  auto dwg = torch::empty_like(wg);
  // transient: the reduce pass hands the gated dy*gamma to the apply pass
  torch::Tensor gsel;
  if (!classic) gsel = torch::empty({B, N, (long)M}, fopt);
  launch_egnmp_bwd(dy.data_ptr(), wg.data_ptr(), idx.data_ptr<int>(),
                   am.data_ptr<unsigned char>(), vsel.data_ptr<float>(),
                   vsum.data_ptr<float>(),
                   offsets.data_ptr<int>(), order_n.data_ptr<int>(),
                   order_j.data_ptr<unsigned char>(),
                   mean.data_ptr<float>(),
                   rstd.data_ptr<float>(), weight.data_ptr<float>(),
                   bias.data_ptr<float>(), scratch.data_ptr<float>(),
                   ws.data_ptr<float>(),
                   classic ? nullptr : gsel.data_ptr<float>(), dwg.data_ptr(),
                   B, N, K, M, (int)G, (int)act, (float)slope, slope_ptr, bf16,
                   rchunks, classic, stream());
  return gn_grads_finish(ws, dwg, rows, M, fopt, wtarget, btarget, starget);
}

// Fused kNN-correlation branch head (csrc/knn_gnmp.hip): conv(4->C) ->
// GroupNorm(G) -> PReLU -> max over K, without the (B, C, K, N)
// intermediate.  raw (B, 4, K, N) fp32; y is (B, N, C) point-major (the
// caller transposes with the narrow-R fast path).
std::vector<torch::Tensor> knn_gnmp_fwd(torch::Tensor raw, torch::Tensor W,
                                        torch::Tensor cb, int64_t G,
                                        torch::Tensor gamma,
                                        torch::Tensor beta, double eps,
                                        torch::Tensor slope_t,
                                        bool out_bf16,
                                        bool channel_major_out = false) {
  check_f32(raw, "raw");
  check_f32(W, "W");
  check_f32(cb, "cb");
  check_f32(gamma, "gamma");
  check_f32(beta, "beta");
  TORCH_CHECK(raw.dim() == 4 && raw.size(1) == 4, "raw must be (B,4,K,N)");
  TORCH_CHECK(slope_t.numel() == 1 && slope_t.scalar_type() == torch::kFloat32);
  const int B = raw.size(0), K = raw.size(2);
  const long N = raw.size(3);
  const int C = W.size(0);
  TORCH_CHECK(W.dim() == 2 && W.size(1) == 4, "W must be (C,4)");
  TORCH_CHECK(C % 16 == 0 && C % G == 0 && C / G >= 4 && K <= 255,
              "knn_gnmp: need C % 16 == 0, C/G >= 4, K <= 255");
  auto fopt = raw.options();
  const int rows = B * (int)G;
  auto& ws = persistent_ws((long)rows * 2, fopt);
  int nblk = (int)((N + 255) / 256);
  if (nblk < 1) nblk = 1;
  const int chunks_f = C / 4;
  // transient (write-then-read within this enqueued call): persistent
  // buffers, NOT per-call pool allocations -- inside a captured training
  // step the per-call workspaces (~85 MB x 12 calls) push the graph pool
  // into the ROCm page-mapping-bug regime (silent garbage at replay;
  // the op alone replays clean, scripts/graph_kg_repro.py)
  auto scratch = persistent_ws((long)rows * 2 * nblk * chunks_f * B, fopt)
                     .view({(long)rows * 2, (long)nblk * chunks_f * B});
  auto mean = torch::empty({rows}, fopt);
  auto rstd = torch::empty({rows}, fopt);
  auto vmax = torch::empty({B, N, C}, fopt);
  auto vmin = torch::empty({B, N, C}, fopt);
  auto vsel = torch::empty({B, N, C}, fopt);
  auto amax = torch::empty({B, N, C}, raw.options().dtype(torch::kUInt8));
  auto amin = torch::empty({B, N, C}, raw.options().dtype(torch::kUInt8));
  auto am = torch::empty({B, N, C}, raw.options().dtype(torch::kUInt8));
  auto yopt = raw.options().dtype(out_bf16 ? torch::kBFloat16
                                           : torch::kFloat32);
  auto y = channel_major_out ? torch::empty({B, (long)C, N}, yopt)
                             : torch::empty({B, N, (long)C}, yopt);
  launch_kg_fwd(raw.data_ptr<float>(), W.data_ptr<float>(),
                cb.data_ptr<float>(), scratch.data_ptr<float>(),
                ws.data_ptr<float>(), mean.data_ptr<float>(),
                rstd.data_ptr<float>(), gamma.data_ptr<float>(),
                beta.data_ptr<float>(), vmax.data_ptr<float>(),
                vmin.data_ptr<float>(), amax.data_ptr<unsigned char>(),
                amin.data_ptr<unsigned char>(), y.data_ptr(),
                am.data_ptr<unsigned char>(), vsel.data_ptr<float>(), B, N,
                K, C, (int)G, (float)eps, slope_t.data_ptr<float>(),
                out_bf16, nblk, channel_major_out, stream());
  return {y, am, vsel, mean, rstd};
}

// dy: the pooled gradient in the layout it arrives in, (B, C, N) when
// dy_channel_major else (B, N, C).  With the five accumulate targets (the
// parameters' fp32 grad buffers) the parameter gradients are added into
// them in-stream and only {draw} is returned; without, {draw, dW, dcb,
// dgamma, dbeta, dslope}.
std::vector<torch::Tensor> knn_gnmp_bwd(
    torch::Tensor dy, torch::Tensor raw, torch::Tensor W, torch::Tensor cb,
    torch::Tensor am, torch::Tensor vsel, torch::Tensor mean,
    torch::Tensor rstd, int64_t G, torch::Tensor gamma, torch::Tensor beta,
    torch::Tensor slope_t, double eps, bool dy_channel_major = false,
    c10::optional<torch::Tensor> wtarget = c10::nullopt,
    c10::optional<torch::Tensor> cbtarget = c10::nullopt,
    c10::optional<torch::Tensor> gtarget = c10::nullopt,
    c10::optional<torch::Tensor> btarget = c10::nullopt,
    c10::optional<torch::Tensor> starget = c10::nullopt) {
  check_f32(raw, "raw");
  check_f32(W, "W");
  check_f32(cb, "cb");
  check_f32(vsel, "vsel");
  check_f32(gamma, "gamma");
  check_f32(beta, "beta");
  TORCH_CHECK(raw.dim() == 4 && raw.size(1) == 4, "raw must be (B,4,K,N)");
  const int B = raw.size(0), K = raw.size(2);
  const long N = raw.size(3);
  const int C = W.size(0);
  TORCH_CHECK(C % 16 == 0 && C <= 128 && G >= 1 && C % G == 0 &&
                  C / G >= 4 && K >= 1 && K <= 255 && N >= 1,
              "knn_gnmp_bwd: need C % 16 == 0, C <= 128, C/G >= 4, "
              "1 <= K <= 255");
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 3 &&
                  dy.size(0) == B &&
                  dy.size(1) == (dy_channel_major ? (long)C : N) &&
                  dy.size(2) == (dy_channel_major ? N : (long)C),
              "dy must be contiguous (B,C,N) or (B,N,C) as flagged");
  const bool bf16 = dy.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || dy.scalar_type() == torch::kFloat32, "fp32/bf16 only");
  TORCH_CHECK(am.is_contiguous() && am.scalar_type() == torch::kUInt8 &&
                  am.numel() == (long)B * N * C && vsel.numel() == am.numel(),
              "am/vsel must be (B,N,C)");
  TORCH_CHECK(mean.numel() == B * G && rstd.numel() == B * G &&
                  slope_t.numel() == 1,
              "mean/rstd/slope shape mismatch");
  auto fopt = raw.options();
  // transient call-internal workspaces: persistent (see knn_gnmp_fwd), one
  // role each so no two of them alias at any shape.  Every element read is
  // written earlier in the same call, so none needs zeroing.  draw (the
  // returned gradient) and the fresh parameter gradients stay per-call:
  // autograd's execution order gives no cross-node liveness guarantee for
  // returned gradients.
  const long bcn = (long)B * C * N;
  auto part = persistent_ws_role("kg_bwd_part", kg_bwd_part_len(B, N, C, G),
                                 fopt);
  auto coef = persistent_ws_role("kg_bwd_coef", (long)B * 20, fopt);
  auto pgrad = persistent_ws_role("kg_bwd_pgrad", kg_bwd_pgrad_len(B, C), fopt);
  auto gsT = persistent_ws_role("kg_bwd_gs", bcn, fopt);
  auto amT = persistent_ws_role("kg_bwd_am", (bcn + 3) / 4, fopt);
  auto draw = torch::empty({B, 4, K, N}, fopt);
  const bool acc = wtarget.has_value();
  torch::Tensor dW, dcb, dgamma, dbeta, dslope;
  if (acc) {
    TORCH_CHECK(cbtarget.has_value() && gtarget.has_value() &&
                    btarget.has_value() && starget.has_value(),
                "knn_gnmp_bwd: all five accumulate targets or none");
    dW = *wtarget;
    dcb = *cbtarget;
    dgamma = *gtarget;
    dbeta = *btarget;
    dslope = *starget;
    check_f32(dW, "wtarget");
    check_f32(dcb, "cbtarget");
    check_f32(dgamma, "gtarget");
    check_f32(dbeta, "btarget");
    check_f32(dslope, "starget");
    TORCH_CHECK(dW.numel() == (long)C * 4 && dcb.numel() == C &&
                    dgamma.numel() == C && dbeta.numel() == C &&
                    dslope.numel() == 1,
                "knn_gnmp_bwd: accumulate target sizes");
  } else {
    dW = torch::empty({C, 4}, fopt);
    dcb = torch::empty({C}, fopt);
    dgamma = torch::empty({C}, fopt);
    dbeta = torch::empty({C}, fopt);
    dslope = torch::empty({1}, fopt);
  }
  launch_kg_bwd(dy.data_ptr(), dy_channel_major, raw.data_ptr<float>(),
                W.data_ptr<float>(), cb.data_ptr<float>(),
                am.data_ptr<unsigned char>(), vsel.data_ptr<float>(),
                mean.data_ptr<float>(), rstd.data_ptr<float>(),
                gamma.data_ptr<float>(), beta.data_ptr<float>(),
                part.data_ptr<float>(), coef.data_ptr<float>(),
                (double*)pgrad.data_ptr<float>(), gsT.data_ptr<float>(), (unsigned char*)amT.data_ptr<float>(),
                draw.data_ptr<float>(), dW.data_ptr<float>(),
                dcb.data_ptr<float>(), dgamma.data_ptr<float>(),
                dbeta.data_ptr<float>(), dslope.data_ptr<float>(), acc, B, N,
                K, C, (int)G, (float)eps, slope_t.data_ptr<float>(), bf16,
                stream());
  if (acc) return {draw};
  return {draw, dW, dcb, dgamma, dbeta, dslope};
}

// Capture-safe batched fp32->bf16 mirror refresh (csrc/cast_pack.hip):
// pointer tables ride kernel arguments, so a hipGraph replay re-reads the
// live fp32 weights (ATen _foreach_copy_'s staging upload does not).
void multi_cast_bf16(std::vector<torch::Tensor> srcs,
                     std::vector<torch::Tensor> dsts) {
  const int n = (int)srcs.size();
  TORCH_CHECK((int)dsts.size() == n, "src/dst count mismatch");
  std::vector<CastChunk> chunks;
  chunks.reserve((n + 127) / 128);
  CastChunk cur;
  cur.count = 0;
  for (int i = 0; i < n; ++i) {
    auto& s = srcs[i];
    auto& d = dsts[i];
    TORCH_CHECK(s.is_cuda() && s.is_contiguous() &&
                s.scalar_type() == torch::kFloat32, "src must be fp32 contig");
    TORCH_CHECK(d.is_cuda() && d.is_contiguous() &&
                d.scalar_type() == torch::kBFloat16 && d.numel() == s.numel(),
                "dst must be matching bf16");
    cur.d[cur.count++] = CastDesc{s.data_ptr<float>(), d.data_ptr(),
                                  (int)s.numel()};
    if (cur.count == 128) {
      chunks.push_back(cur);
      cur.count = 0;
    }
  }
  if (cur.count) chunks.push_back(cur);
  if (!chunks.empty())
    launch_multi_cast(chunks.data(), (int)chunks.size(), stream());
}

// dy (B, Co, S) bf16, x (B, Ci, S) bf16 -> dW (Co, Ci) fp32 (split-K MFMA)
std::vector<torch::Tensor> pw_wgrad(torch::Tensor dy, torch::Tensor x,
                                    int64_t schunks = 0, bool with_bias = false) {
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 3);
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 3);
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 && x.scalar_type() == torch::kBFloat16,
              "pw_wgrad is bf16-only");
  TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(2) == x.size(2), "shape mismatch");
  const int B = dy.size(0), Co = dy.size(1), Ci = x.size(1);
  const long S = dy.size(2);
  // dw and dbias share one zeroed allocation (both are atomic-accumulated;
  // a two-stage partial-store + reduce variant measured 2x SLOWER -- the
  // partial-buffer write+read traffic dwarfs the L2 atomics on this tiny
  // output, scripts/kernel_bench.py)
  auto flat = zeros_fast({(long)Co * Ci + (with_bias ? Co : 0)},
                         dy.options().dtype(torch::kFloat32));
  auto dw = flat.narrow(0, 0, (long)Co * Ci).view({Co, Ci});
  torch::Tensor dbias;
  float* dbias_ptr = nullptr;
  if (with_bias) {
    dbias = flat.narrow(0, (long)Co * Ci, Co);
    dbias_ptr = dbias.data_ptr<float>();
  }
  launch_pw_wgrad(dy.data_ptr(), x.data_ptr(), dw.data_ptr<float>(), dbias_ptr,
                  B, Co, Ci, S, (int)schunks, stream());
  return {dw, dbias};
}

// Fused MFMA 1x1-conv forward: y = act(sum_i W_i @ x_i + bias + addend)
// in one launch (csrc/pw_fwd.hip)
void launch_pw_fwd(const void**, const void**, const int*, const int*, int,
                   const float*, const void*, long, int, void*, int, int, long,
                   int, int, hipStream_t);

torch::Tensor pw_fwd(std::vector<torch::Tensor> ws,
                     std::vector<torch::Tensor> xs,
                     c10::optional<torch::Tensor> bias,
                     c10::optional<torch::Tensor> addend, int64_t act,
                     bool point_major = false) {
  const int n = (int)ws.size();
  TORCH_CHECK(n >= 1 && n <= 4 && (int)xs.size() == n, "1..4 parts");
  const int Co = ws[0].size(0);
  const int B = xs[0].size(0);
  const long S = xs[0].size(2);
  const void* wp[4];
  const void* xp[4];
  int cis[4];
  int lds[4];
  for (int i = 0; i < n; ++i) {
    // rows contiguous, any row pitch: column slices of a wider weight
    TORCH_CHECK(ws[i].is_cuda() && ws[i].dim() == 2 &&
                (ws[i].size(1) == 1 || ws[i].stride(1) == 1) &&
                (ws[i].size(0) == 1 || ws[i].stride(0) >= ws[i].size(1)) &&
                ws[i].scalar_type() == torch::kBFloat16,
                "w must be (Co,Ci) bf16 with contiguous rows");
    TORCH_CHECK(xs[i].is_cuda() && xs[i].is_contiguous() && xs[i].dim() == 3 &&
                xs[i].scalar_type() == torch::kBFloat16, "x must be (B,Ci,S) bf16");
    TORCH_CHECK(ws[i].size(0) == Co && xs[i].size(0) == B && xs[i].size(2) == S);
    TORCH_CHECK(ws[i].size(1) == xs[i].size(1), "w/x channel mismatch");
    TORCH_CHECK(ws[i].size(1) <= 224, "pw_fwd: Ci <= 224");
    wp[i] = ws[i].data_ptr();
    xp[i] = xs[i].data_ptr();
    cis[i] = (int)ws[i].size(1);
    lds[i] = ws[i].size(0) == 1 ? cis[i] : (int)ws[i].stride(0);
  }
  TORCH_CHECK(Co <= 256, "pw_fwd: Co <= 256");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->scalar_type() == torch::kFloat32 && bias->is_contiguous() &&
                bias->numel() == Co, "bias must be fp32 (Co)");
    bptr = bias->data_ptr<float>();
  }
  const void* aptr = nullptr;
  long abstride = 0;
  int afp32 = 0;
  if (addend.has_value() && addend->defined()) {
    auto& a = *addend;
    TORCH_CHECK(a.is_cuda() && a.dim() == 3 && a.size(0) == B &&
                a.size(1) == Co && a.size(2) == S, "addend must be (B,Co,S) view");
    TORCH_CHECK(a.stride(2) == 1 && a.stride(1) == S,
                "addend rows must be contiguous");
    afp32 = a.scalar_type() == torch::kFloat32;
    TORCH_CHECK(afp32 || a.scalar_type() == torch::kBFloat16, "addend fp32/bf16");
    aptr = a.data_ptr();
    abstride = a.stride(0);
  }
  // point_major: y is written (B, S, Co) straight from the epilogue
  auto y = point_major ? torch::empty({B, S, (long)Co}, xs[0].options())
                       : torch::empty({B, (long)Co, S}, xs[0].options());
  launch_pw_fwd(wp, xp, cis, lds, n, bptr, aptr, abstride, afp32, y.data_ptr(), B,
                Co, S, (int)act, point_major ? 1 : 0, stream());
  return y;
}

// Fused data gradient of a pw_fwd stack (csrc/pw_bwd.hip): ReLU mask,
// point-major transpose and every part's W_i^T @ dpre in one launch.
// Returns the dx of the wanted parts in order, then dpre (channel-major;
// dy itself when neither ReLU nor point-major changes it, the slab's row
// block when a slab is given).
void launch_pw_bwd(const void**, void**, const int*, const int*, int,
                   const void*, const void*, void*, long, int, int, long, int,
                   hipStream_t);

std::vector<torch::Tensor> pw_bwd(torch::Tensor dy,
                                  c10::optional<torch::Tensor> y,
                                  std::vector<torch::Tensor> ws,
                                  std::vector<bool> want, int64_t act,
                                  bool point_major,
                                  c10::optional<torch::Tensor> slab,
                                  int64_t r0) {
  const int n = (int)ws.size();
  TORCH_CHECK(n <= 4 && (int)want.size() == n, "pw_bwd: at most 4 parts");
  TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 3 &&
              dy.scalar_type() == torch::kBFloat16,
              "pw_bwd: dy must be contiguous 3-D bf16");
  const int B = dy.size(0);
  const int Co = point_major ? dy.size(2) : dy.size(1);
  const long S = point_major ? dy.size(1) : dy.size(2);
  TORCH_CHECK(Co >= 1 && Co <= 256, "pw_bwd: Co <= 256");
  TORCH_CHECK(act == 0 || act == 1, "pw_bwd: act 0 (none) or 1 (relu)");
  const void* yptr = nullptr;
  if (act == 1) {
    TORCH_CHECK(y.has_value() && y->defined() && y->is_cuda() &&
                y->is_contiguous() && y->scalar_type() == torch::kBFloat16 &&
                y->sizes() == dy.sizes(),
                "pw_bwd: relu needs the saved y, shaped like dy");
    yptr = y->data_ptr();
  }
  const void* wp[4];
  void* dxp[4];
  int cis[4];
  int lds[4];
  std::vector<torch::Tensor> outs;
  int nw = 0;
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(ws[i].is_cuda() && ws[i].dim() == 2 &&
                (ws[i].size(1) == 1 || ws[i].stride(1) == 1) &&
                (ws[i].size(0) == 1 || ws[i].stride(0) >= ws[i].size(1)) &&
                ws[i].scalar_type() == torch::kBFloat16,
                "w must be (Co,Ci) bf16 with contiguous rows");
    TORCH_CHECK(ws[i].size(0) == Co, "pw_bwd: w rows != Co");
    TORCH_CHECK(ws[i].size(1) >= 1 && ws[i].size(1) <= 224, "pw_bwd: Ci <= 224");
    if (!want[i]) continue;
    const long Ci = ws[i].size(1);
    auto dx = torch::empty({B, Ci, S}, dy.options());
    wp[nw] = ws[i].data_ptr();
    dxp[nw] = dx.data_ptr();
    cis[nw] = (int)Ci;
    lds[nw] = ws[i].size(0) == 1 ? (int)Ci : (int)ws[i].stride(0);
    outs.push_back(dx);
    ++nw;
  }
  torch::Tensor dpre = dy;
  void* dptr = nullptr;
  long dbs = 0;
  if (slab.has_value() && slab->defined()) {
    auto& sl = *slab;
    TORCH_CHECK(act == 0 && !point_major,
                "pw_bwd: slab output needs act=none and channel-major dy");
    TORCH_CHECK(sl.is_cuda() && sl.dim() == 3 && sl.size(0) == B &&
                sl.size(2) == S && sl.scalar_type() == torch::kBFloat16 &&
                sl.stride(2) == 1 && sl.stride(1) == S &&
                r0 >= 0 && r0 + Co <= sl.size(1),
                "pw_bwd: slab must be (B,Ctot,S) bf16 with contiguous rows");
    dpre = sl.narrow(1, r0, Co);
    dptr = dpre.data_ptr();
    dbs = sl.stride(0);
  } else if (act == 1 || point_major) {
    dpre = torch::empty({B, (long)Co, S}, dy.options());
    dptr = dpre.data_ptr();
    dbs = (long)Co * S;
  }
  if (B > 0 && S > 0 && (nw > 0 || dptr != nullptr))
    launch_pw_bwd(wp, dxp, cis, lds, nw, dy.data_ptr(), yptr, dptr, dbs, B, Co,
                  S, point_major ? 1 : 0, stream());
  outs.push_back(dpre);
  return outs;
}

// Batched deferred weight gradients: many (dy, x) -> dW problems in ONE
// kernel launch, each ACCUMULATED into its weight's existing fp32 grad
// buffer (no per-call zero-fill, no autograd accumulate-add).  ~180 such
// problems per train step (the GRU loop's conv stacks) were
// launch/atomic-floor-bound when launched one-by-one.
// dbs entries with numel 0 mean "no bias gradient for this job".
// Returns {host_desc, dev_desc} -- the caller must keep both alive while a
// hipGraph captured over this call can still replay (the recorded H2D copy
// re-reads the pinned host buffer).
#include "pw_wgrad_job.h"
void launch_pw_wgrad_batched(const void*, const unsigned int*, int,
                             hipStream_t);
void launch_desc_fill(void*, const void*, long, hipStream_t);

std::vector<torch::Tensor> pw_wgrad_batched(std::vector<torch::Tensor> dys,
                                            std::vector<torch::Tensor> xs,
                                            std::vector<torch::Tensor> dws,
                                            std::vector<torch::Tensor> dbs) {
  const int n = (int)dys.size();
  TORCH_CHECK(n >= 1 && n <= 4095, "1..4095 jobs");
  TORCH_CHECK((int)xs.size() == n && (int)dws.size() == n && (int)dbs.size() == n);
  std::vector<PwWgradJob> jobs(n);
  long base_blocks = 0;
  const int TILE = 64;
  for (int j = 0; j < n; ++j) {
    auto& dy = dys[j];
    auto& x = xs[j];
    auto& dw = dws[j];
    TORCH_CHECK(dy.is_cuda() && dy.is_contiguous() && dy.dim() == 3 &&
                dy.scalar_type() == torch::kBFloat16, "dy must be (B,Co,S) bf16");
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 3 &&
                x.scalar_type() == torch::kBFloat16, "x must be (B,Ci,S) bf16");
    TORCH_CHECK(dy.size(0) == x.size(0) && dy.size(2) == x.size(2), "dy/x mismatch");
    // flat contiguous, or a (Co, Ci) column block of a wider grad buffer
    // (rows contiguous, row pitch >= Ci)
    const bool dw_block = dw.dim() == 2 && !dw.is_contiguous();
    TORCH_CHECK(dw.is_cuda() && dw.scalar_type() == torch::kFloat32 &&
                (dw_block ? (dw.stride(1) == 1 && dw.stride(0) >= dw.size(1))
                          : dw.is_contiguous()),
                "dw must be fp32, contiguous or a row-contiguous block");
    const int Co = dy.size(1), Ci = x.size(1);
    TORCH_CHECK(dw.numel() == (long)Co * Ci &&
                (!dw_block || (dw.size(0) == Co && dw.size(1) == Ci)),
                "dw shape mismatch");
    const int ldw = dw_block ? (int)dw.stride(0) : Ci;
    TORCH_CHECK(Co <= 16 * TILE && Ci <= 16 * TILE, "Co/Ci too large for 4-bit tile index");
    float* dbias = nullptr;
    if (dbs[j].defined() && dbs[j].numel() > 0) {
      TORCH_CHECK(dbs[j].is_cuda() && dbs[j].is_contiguous() &&
                  dbs[j].scalar_type() == torch::kFloat32 && dbs[j].numel() == Co);
      dbias = dbs[j].data_ptr<float>();
    }
    jobs[j] = PwWgradJob{dy.data_ptr(), x.data_ptr(), dw.data_ptr<float>(),
                         dbias, Co, Ci, (int)dy.size(0), 1, dy.size(2), ldw,
                         0};
    base_blocks += (long)((Co + TILE - 1) / TILE) * ((Ci + TILE - 1) / TILE) *
                   dy.size(0);
  }
  // split each job's reduction so every block gets ~96 K-loop iterations
  // (~3072 reduction elements): a single global split starved the few
  // huge-S jobs (S ~ 262k, the kNN-branch convs), whose straggler blocks
  // then dominated the whole launch
  (void)base_blocks;
  for (int j = 0; j < n; ++j) {
    long sc = (jobs[j].S + 3071) / 3072;
    if (sc < 1) sc = 1;
    if ((long)jobs[j].B * sc > 4095) sc = 4095 / jobs[j].B;
    jobs[j].schunks = (int)sc;
  }
  std::vector<unsigned int> map;
  map.reserve(4096);
  for (int j = 0; j < n; ++j) {
    const int to = (jobs[j].Co + TILE - 1) / TILE;
    const int ti = (jobs[j].Ci + TILE - 1) / TILE;
    const int bzs = jobs[j].B * jobs[j].schunks;
    for (int bz = 0; bz < bzs; ++bz)
      for (int a = 0; a < to; ++a)
        for (int b = 0; b < ti; ++b)
          map.push_back(((unsigned)j << 20) | ((unsigned)bz << 8) |
                        ((unsigned)a << 4) | (unsigned)b);
  }
  const long jbytes = (long)n * sizeof(PwWgradJob);
  const long mbytes = (long)map.size() * sizeof(unsigned int);
  std::vector<unsigned char> blob(jbytes + mbytes);
  memcpy(blob.data(), jobs.data(), jbytes);
  memcpy(blob.data() + jbytes, map.data(), mbytes);
  auto dev = torch::empty({jbytes + mbytes}, dys[0].options().dtype(torch::kUInt8));
  // descriptor bytes travel as kernel ARGUMENTS (desc_fill_kernel): plain
  // launches that hipGraph capture records like any other kernel -- no
  // H2D memcpy / events / pinned memory, which all invalidate capture on
  // this stack.  Outside capture the same path is a handful of ~2 us
  // launches.
  launch_desc_fill(dev.data_ptr(), blob.data(), jbytes + mbytes, stream());
  launch_pw_wgrad_batched(dev.data_ptr(),
                          (const unsigned int*)((char*)dev.data_ptr() + jbytes),
                          (int)map.size(), stream());
  // caller keeps dev alive for the lifetime of any capturing graph
  return {dev};
}

// (B, R, C) view (row-contiguous, arbitrary batch stride) -> (B, C, R)
torch::Tensor batched_transpose(torch::Tensor x) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 3, "x must be 3-D GPU");
  TORCH_CHECK(x.stride(2) == 1 && x.stride(1) == x.size(2),
              "rows must be contiguous");
  const bool bf16 = x.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || x.scalar_type() == torch::kFloat32, "fp32/bf16 only");
  const int B = x.size(0);
  const long R = x.size(1), C = x.size(2);
  auto out = torch::empty({B, C, R}, x.options());
  launch_transpose(x.data_ptr(), out.data_ptr(), x.stride(0), B, R, C, bf16,
                   stream());
  return out;
}

std::vector<torch::Tensor> pv_corr_fused_fwd(torch::Tensor corr,
                                             torch::Tensor xyz,
                                             torch::Tensor coords,
                                             double base_scale,
                                             int64_t num_levels, int64_t k) {
  check_f32(corr, "corr");
  check_f32(xyz, "xyz");
  check_f32(coords, "coords");
  const int B = corr.size(0), N = corr.size(1), K = corr.size(2);
  TORCH_CHECK(K <= 512 && num_levels >= 1 && num_levels <= 4 && k >= 1 && k <= 64 && k <= K);
  auto vox = torch::empty({B, num_levels * 27, N}, corr.options());
  auto knn = torch::empty({B, 4, k, N}, corr.options());
  auto idx = torch::empty({B, N, k}, corr.options().dtype(torch::kInt32));
  launch_pv_corr_fused_fwd(corr.data_ptr<float>(), xyz.data_ptr<float>(),
                           coords.data_ptr<float>(), vox.data_ptr<float>(),
                           knn.data_ptr<float>(), idx.data_ptr<int>(), B, N, K,
                           (int)num_levels, (int)k, (float)base_scale, stream());
  return {vox, knn, idx};
}

torch::Tensor pv_corr_fused_bwd(torch::Tensor g_vox, torch::Tensor g_knn,
                                torch::Tensor xyz, torch::Tensor coords,
                                torch::Tensor knn_idx, int64_t num_levels,
                                int64_t k, double base_scale) {
  check_f32(g_vox, "g_vox");
  check_f32(g_knn, "g_knn");
  const int B = xyz.size(0), N = xyz.size(1), K = xyz.size(2);
  auto gcorr = torch::empty({B, N, K}, g_vox.options());
  launch_pv_corr_fused_bwd(g_vox.data_ptr<float>(), g_knn.data_ptr<float>(),
                           xyz.data_ptr<float>(), coords.data_ptr<float>(),
                           knn_idx.data_ptr<int>(), gcorr.data_ptr<float>(), B,
                           N, K, (int)num_levels, (int)k, (float)base_scale,
                           stream());
  return gcorr;
}

// Fused bf16 MFMA correlation GEMM + streaming top-K truncation
// (reference corr.py:95-99 + corr.py:37): f1t (B,N,C), f2t (B,M,C) bf16
// point-major -> top-K values (B,N,K) fp32 + indices (B,N,K) i32; the
// (N, M) correlation matrix is never materialised.  Top-K SET is
// unordered (all consumers are order-invariant).
void launch_corr_topk(const void*, const void*, float*, float*, int*, float*,
                      int*, int*, int, int, int, int, int, float,
                      hipStream_t);

std::vector<torch::Tensor> corr_topk(torch::Tensor f1t, torch::Tensor f2t,
                                     int64_t K) {
  TORCH_CHECK(f1t.is_cuda() && f1t.is_contiguous() && f1t.dim() == 3 &&
              f1t.scalar_type() == torch::kBFloat16, "f1t must be (B,N,C) bf16");
  TORCH_CHECK(f2t.is_cuda() && f2t.is_contiguous() && f2t.dim() == 3 &&
              f2t.scalar_type() == torch::kBFloat16, "f2t must be (B,M,C) bf16");
  const int B = f1t.size(0), N = f1t.size(1), C = f1t.size(2);
  const int M = f2t.size(1);
  TORCH_CHECK(f2t.size(0) == B && f2t.size(2) == C, "f1t/f2t mismatch");
  TORCH_CHECK(C % 32 == 0 && C <= 256, "need C % 32 == 0, C <= 256");
  TORCH_CHECK(K >= 1 && K <= M && K <= 1024, "need 1 <= K <= min(M, 1024)");
  auto fopt = f1t.options().dtype(torch::kFloat32);
  auto iopt = f1t.options().dtype(torch::kInt32);
  const long R = (long)B * N;
  auto thr = torch::empty({R, 2}, fopt);
  auto out_v = torch::empty({B, (long)N, K}, fopt);
  auto out_i = torch::empty({B, (long)N, K}, iopt);
  auto band_v = torch::empty({R, 704}, fopt);
  auto band_i = torch::empty({R, 704}, iopt);
  auto cnt = zeros_fast({R, 2}, iopt);
  launch_corr_topk(f1t.data_ptr(), f2t.data_ptr(), thr.data_ptr<float>(),
                   out_v.data_ptr<float>(), out_i.data_ptr<int>(),
                   band_v.data_ptr<float>(), band_i.data_ptr<int>(),
                   cnt.data_ptr<int>(), B, N, M, C, (int)K,
                   1.0f / sqrtf((float)C), stream());
  return {out_v, out_i};
}

void launch_corr_grad_expand(const float*, const int*, void*, long, int, int,
                             float, bool, hipStream_t);
void launch_corr_gather_xyz(const int*, const float*, float*, int, long, int,
                            hipStream_t);

// g (B,N,K) fp32, idx (B,N,K) i32 -> dense (B,N,M) bf16 / fp32 with
// round(g * scale) at idx and zeros elsewhere; every element stored once
// (csrc/corr_bwd.hip).  The row image lives in LDS: M * itemsize <= 64 KB.
torch::Tensor corr_grad_expand(torch::Tensor g, torch::Tensor idx,
                               double scale, int64_t M, bool bf16) {
  check_f32(g, "g");
  TORCH_CHECK(g.dim() == 3, "g must be (B, N, K)");
  TORCH_CHECK(idx.is_cuda() && idx.is_contiguous() &&
              idx.scalar_type() == torch::kInt32 && idx.sizes() == g.sizes(),
              "idx must be contiguous int32 of g's shape");
  TORCH_CHECK(idx.device() == g.device(), "g and idx on different devices");
  TORCH_CHECK(M >= 1 && M * (bf16 ? 2 : 4) <= 64 * 1024,
              "row image limited to 64 KB");
  const long B = g.size(0), N = g.size(1);
  TORCH_CHECK(B * N < (1L << 31), "too many rows");
  auto out = torch::empty(
      {B, N, M}, g.options().dtype(bf16 ? torch::kBFloat16 : torch::kFloat32));
  launch_corr_grad_expand(g.data_ptr<float>(), idx.data_ptr<int>(),
                          out.data_ptr(), B * N, (int)g.size(2), (int)M,
                          (float)scale, bf16, stream());
  return out;
}

// idx (B,N,K) i32, xyz2 (B,M,3) fp32 -> xyz2 rows at idx, (B,N,K,3) fp32
torch::Tensor corr_gather_xyz(torch::Tensor idx, torch::Tensor xyz2) {
  check_f32(xyz2, "xyz2");
  TORCH_CHECK(idx.is_cuda() && idx.is_contiguous() && idx.dim() == 3 &&
              idx.scalar_type() == torch::kInt32,
              "idx must be contiguous (B, N, K) int32");
  TORCH_CHECK(xyz2.dim() == 3 && xyz2.size(2) == 3 &&
              xyz2.size(0) == idx.size(0) && xyz2.size(1) >= 1,
              "xyz2 must be (B, M, 3)");
  TORCH_CHECK(idx.device() == xyz2.device(),
              "idx and xyz2 on different devices");
  const long B = idx.size(0), N = idx.size(1), K = idx.size(2);
  TORCH_CHECK((B * N * K + 1023) / 1024 < (1L << 31), "too many entries");
  auto out = torch::empty({B, N, K, 3}, xyz2.options());
  launch_corr_gather_xyz(idx.data_ptr<int>(), xyz2.data_ptr<float>(),
                         out.data_ptr<float>(), (int)B, N * K,
                         (int)xyz2.size(1), stream());
  return out;
}

// vals (R, M) fp32 -> top-K largest per row: values (R, K), idx (R, K)
std::vector<torch::Tensor> topk_rows(torch::Tensor vals, int64_t K) {
  check_f32(vals, "vals");
  TORCH_CHECK(vals.dim() == 2, "vals must be (R, M)");
  const long R = vals.size(0);
  const int M = vals.size(1);
  TORCH_CHECK(M <= 8192, "topk_rows supports M <= 8192");
  TORCH_CHECK(K >= 1 && K <= M, "need 1 <= K <= M");
  auto out_v = torch::empty({R, K}, vals.options());
  auto out_i = torch::empty({R, K}, vals.options().dtype(torch::kInt32));
  launch_topk_rows(vals.data_ptr<float>(), out_v.data_ptr<float>(),
                   out_i.data_ptr<int>(), R, M, (int)K, stream());
  return {out_v, out_i};
}

namespace {

void check_gru(const torch::Tensor& t, const torch::Tensor& like,
               const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == like.scalar_type(), name,
              " dtype mismatch in fused GRU gates");
}

}  // namespace

// pre (B,2H,N) [z|r preactivations], h (B,H,N) -> z, r, rh (each (B,H,N))
std::vector<torch::Tensor> gru_zr_fwd(torch::Tensor pre, torch::Tensor h) {
  TORCH_CHECK(pre.is_cuda() && pre.is_contiguous() && h.is_contiguous());
  TORCH_CHECK(pre.dim() == 3 && h.dim() == 3 && pre.size(0) == h.size(0) &&
              pre.size(1) == 2 * h.size(1) && pre.size(2) == h.size(2));
  const bool bf16 = pre.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || pre.scalar_type() == torch::kFloat32);
  check_gru(h, pre, "h");
  auto z = torch::empty_like(h), r = torch::empty_like(h),
       rh = torch::empty_like(h);
  launch_gru_zr_fwd(pre.data_ptr(), h.data_ptr(), z.data_ptr(), r.data_ptr(),
                    rh.data_ptr(), h.size(0), (long)h.size(1) * h.size(2),
                    bf16, stream());
  return {z, r, rh};
}

std::vector<torch::Tensor> gru_zr_bwd(torch::Tensor dz, torch::Tensor drh,
                                      torch::Tensor z, torch::Tensor r,
                                      torch::Tensor h) {
  const bool bf16 = z.scalar_type() == torch::kBFloat16;
  for (auto* t : {&dz, &drh, &r, &h}) check_gru(*t, z, "gru_zr_bwd input");
  auto dpre = torch::empty({h.size(0), 2 * h.size(1), h.size(2)}, h.options());
  auto dh = torch::empty_like(h);
  launch_gru_zr_bwd(dz.data_ptr(), drh.data_ptr(), z.data_ptr(), r.data_ptr(),
                    h.data_ptr(), dpre.data_ptr(), dh.data_ptr(), h.size(0),
                    (long)h.size(1) * h.size(2), bf16, stream());
  return {dpre, dh};
}

// pre_q, z, h (B,H,N) -> q, hnew
std::vector<torch::Tensor> gru_q_fwd(torch::Tensor pre, torch::Tensor z,
                                     torch::Tensor h) {
  const bool bf16 = pre.scalar_type() == torch::kBFloat16;
  TORCH_CHECK(bf16 || pre.scalar_type() == torch::kFloat32);
  for (auto* t : {&pre, &z, &h}) check_gru(*t, pre, "gru_q_fwd input");
  auto q = torch::empty_like(h), hnew = torch::empty_like(h);
  launch_gru_q_fwd(pre.data_ptr(), z.data_ptr(), h.data_ptr(), q.data_ptr(),
                   hnew.data_ptr(), h.size(0), (long)h.size(1) * h.size(2),
                   bf16, stream());
  return {q, hnew};
}

std::vector<torch::Tensor> gru_q_bwd(torch::Tensor dhnew, torch::Tensor q,
                                     torch::Tensor z, torch::Tensor h) {
  const bool bf16 = q.scalar_type() == torch::kBFloat16;
  for (auto* t : {&dhnew, &z, &h}) check_gru(*t, q, "gru_q_bwd input");
  auto dpre = torch::empty_like(h), dz = torch::empty_like(h),
       dh = torch::empty_like(h);
  launch_gru_q_bwd(dhnew.data_ptr(), q.data_ptr(), z.data_ptr(), h.data_ptr(),
                   dpre.data_ptr(), dz.data_ptr(), dh.data_ptr(), h.size(0),
                   (long)h.size(1) * h.size(2), bf16, stream());
  return {dpre, dz, dh};
}

// fused gamma-weighted sequence loss over T flows -> {loss, denom}
std::vector<torch::Tensor> seq_loss_fwd(std::vector<torch::Tensor> flows,
                                        torch::Tensor gt, torch::Tensor mask,
                                        double gamma) {
  const int T = (int)flows.size();
  TORCH_CHECK(T >= 1 && T <= 32, "seq_loss supports 1..32 flows");
  check_f32(gt, "gt");
  check_f32(mask, "mask");
  const long BN = gt.numel() / 3;
  TORCH_CHECK(mask.numel() == BN, "mask/gt shape mismatch");
  const float* ptrs[32];
  for (int t = 0; t < T; ++t) {
    check_f32(flows[t], "flow");
    TORCH_CHECK(flows[t].numel() == BN * 3, "flow shape mismatch");
    ptrs[t] = flows[t].data_ptr<float>();
  }
  auto fopt = gt.options();
  // persistent self-cleaning workspace (finalize re-zeroes); leaked on
  // purpose so its destructor never races CUDA teardown at exit
  static torch::Tensor* ws_p = new torch::Tensor();
  torch::Tensor& ws = *ws_p;
  if (!ws.defined()) ws = torch::zeros({33}, fopt);
  auto loss = torch::empty({}, fopt);
  auto denom = torch::empty({}, fopt);
  launch_seq_loss_fwd(ptrs, gt.data_ptr<float>(), mask.data_ptr<float>(),
                      ws.data_ptr<float>(), loss.data_ptr<float>(),
                      denom.data_ptr<float>(), BN, T, 1, (float)gamma,
                      stream());
  return {loss, denom};
}

std::vector<torch::Tensor> seq_loss_bwd(std::vector<torch::Tensor> flows,
                                        torch::Tensor gt, torch::Tensor mask,
                                        torch::Tensor dloss,
                                        torch::Tensor denom, double gamma) {
  const int T = (int)flows.size();
  TORCH_CHECK(T >= 1 && T <= 32);
  const long BN = gt.numel() / 3;
  const float* ptrs[32];
  float* gptrs[32];
  std::vector<torch::Tensor> grads;
  grads.reserve(T);
  for (int t = 0; t < T; ++t) {
    ptrs[t] = flows[t].data_ptr<float>();
    grads.push_back(torch::empty_like(flows[t]));
    gptrs[t] = grads[t].data_ptr<float>();
  }
  launch_seq_loss_bwd(ptrs, gptrs, gt.data_ptr<float>(),
                      mask.data_ptr<float>(), dloss.data_ptr<float>(),
                      denom.data_ptr<float>(), BN, T, 1, (float)gamma,
                      stream());
  return grads;
}

static void check_i32(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == torch::kInt32,
              name, " must be a contiguous int32 GPU tensor");
}

// shared shape / range checks of the Chamfer entry points
static void chamfer_check(const torch::Tensor& pc1, const torch::Tensor& pc2,
                          int64_t T) {
  check_f32(pc1, "pc1");
  check_f32(pc2, "pc2");
  TORCH_CHECK(pc1.dim() == 3 && pc1.size(2) == 3, "pc1 must be (B,N,3)");
  TORCH_CHECK(pc2.dim() == 3 && pc2.size(2) == 3, "pc2 must be (B,M,3)");
  TORCH_CHECK(pc2.device() == pc1.device(), "chamfer inputs must share a device");
  const int64_t B = pc1.size(0), N = pc1.size(1), M = pc2.size(1);
  TORCH_CHECK(pc2.size(0) == B, "chamfer batch mismatch");
  TORCH_CHECK(T >= 1 && T <= 32, "chamfer supports 1..32 flows");
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1 && M >= 1,
              "chamfer requires 1 <= B <= 65535, N, M >= 1");
  TORCH_CHECK(N < (1L << 31) - 256 && M < (1L << 31) - 256,
              "chamfer sizes exceed 32-bit point indexing");
}

// pc1 (B,N,3), flows (T,B,N,3), pc2 (B,M,3), all fp32 contiguous ->
// {chamfer (T) f32, d2_1 (T,B,N) f32, idx_1 (T,B,N) i32, d2_2 (T,B,M) f32,
//  idx_2 (T,B,M) i32}
std::vector<torch::Tensor> chamfer_fwd(torch::Tensor pc1, torch::Tensor flows,
                                       torch::Tensor pc2) {
  check_f32(flows, "flows");
  TORCH_CHECK(flows.dim() == 4, "flows must be (T,B,N,3)");
  const int64_t T = flows.size(0);
  chamfer_check(pc1, pc2, T);
  const int64_t B = pc1.size(0), N = pc1.size(1), M = pc2.size(1);
  TORCH_CHECK(flows.size(1) == B && flows.size(2) == N && flows.size(3) == 3 &&
                  flows.device() == pc1.device(),
              "flows must be (T,B,N,3) on the device of pc1");
  auto fopt = pc1.options();
  auto iopt = fopt.dtype(torch::kInt32);
  auto d1 = torch::empty({T, B, N}, fopt);
  auto i1 = torch::empty({T, B, N}, iopt);
  auto d2 = torch::empty({T, B, M}, fopt);
  auto i2 = torch::empty({T, B, M}, iopt);
  const int nblk = chamfer_fwd_blocks((int)N, (int)M, 2);
  // blocks past the end of the smaller cloud write nothing: zero-filled
  auto part = torch::zeros({T, 2, B * (int64_t)nblk}, fopt);
  launch_chamfer_fwd(pc1.data_ptr<float>(), flows.data_ptr<float>(),
                     pc2.data_ptr<float>(), d1.data_ptr<float>(),
                     i1.data_ptr<int>(), d2.data_ptr<float>(),
                     i2.data_ptr<int>(), part.data_ptr<float>(), (int)B, (int)N,
                     (int)M, (int)T, 2, stream());
  auto sums = part.sum(2);  // (T, 2), deterministic fold of the block sums
  auto cham = sums.select(1, 0) / (double)(B * N) + sums.select(1, 1) / (double)(B * M);
  return {cham, d1, i1, d2, i2};
}

// one direction, no flow: query (B,Q,3), support (B,S,3) -> {d2 (B,Q), idx (B,Q) i32}
std::vector<torch::Tensor> chamfer_nn_fwd(torch::Tensor query,
                                          torch::Tensor support) {
  chamfer_check(query, support, 1);
  const int64_t B = query.size(0), Q = query.size(1), S = support.size(1);
  auto d = torch::empty({B, Q}, query.options());
  auto i = torch::empty({B, Q}, query.options().dtype(torch::kInt32));
  const int nblk = chamfer_fwd_blocks((int)Q, (int)S, 1);
  auto part = torch::empty({B * (int64_t)nblk}, query.options());
  launch_chamfer_fwd(query.data_ptr<float>(), nullptr,
                     support.data_ptr<float>(), d.data_ptr<float>(),
                     i.data_ptr<int>(), nullptr, nullptr,
                     part.data_ptr<float>(), (int)B, (int)Q, (int)S, 1, 1,
                     stream());
  return {d, i};
}

// gradient of sum_t g_t * chamfer_t with respect to the flows
torch::Tensor chamfer_bwd(torch::Tensor pc1, torch::Tensor flows,
                          torch::Tensor pc2, torch::Tensor idx1,
                          torch::Tensor idx2, torch::Tensor gout) {
  check_f32(flows, "flows");
  check_f32(gout, "grad");
  check_i32(idx1, "idx1");
  check_i32(idx2, "idx2");
  TORCH_CHECK(flows.dim() == 4, "flows must be (T,B,N,3)");
  const int64_t T = flows.size(0);
  chamfer_check(pc1, pc2, T);
  const int64_t B = pc1.size(0), N = pc1.size(1), M = pc2.size(1);
  TORCH_CHECK(flows.size(1) == B && flows.size(2) == N && flows.size(3) == 3,
              "flows must be (T,B,N,3)");
  TORCH_CHECK(idx1.numel() == T * B * N && idx2.numel() == T * B * M &&
                  gout.numel() == T,
              "chamfer_bwd index / gradient shape mismatch");
  TORCH_CHECK(flows.device() == pc1.device() && idx1.device() == pc1.device() &&
                  idx2.device() == pc1.device() && gout.device() == pc1.device(),
              "chamfer_bwd inputs must share a device");
  auto dflow = torch::empty_like(flows);
  launch_chamfer_bwd(pc1.data_ptr<float>(), flows.data_ptr<float>(),
                     pc2.data_ptr<float>(), idx1.data_ptr<int>(),
                     idx2.data_ptr<int>(), gout.data_ptr<float>(),
                     dflow.data_ptr<float>(), (int)B, (int)N, (int)M, (int)T,
                     stream());
  return dflow;
}

static void flow_smooth_check(const torch::Tensor& flows,
                              const torch::Tensor& idx) {
  check_f32(flows, "flows");
  check_i32(idx, "idx");
  TORCH_CHECK(flows.dim() == 4 && flows.size(3) == 3, "flows must be (T,B,N,3)");
  TORCH_CHECK(idx.dim() == 3, "idx must be (B,N,k)");
  const int64_t T = flows.size(0), B = flows.size(1), N = flows.size(2);
  TORCH_CHECK(idx.size(0) == B && idx.size(1) == N && idx.device() == flows.device(),
              "idx must be (B,N,k) on the device of flows");
  TORCH_CHECK(T >= 1 && T <= 32, "flow_smooth supports 1..32 flows");
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1 && idx.size(2) >= 1,
              "flow_smooth requires 1 <= B <= 65535, N, k >= 1");
  TORCH_CHECK(N * idx.size(2) < (1L << 31) - 256,
              "flow_smooth sizes exceed 32-bit edge indexing");
}

// flows (T,B,N,3) f32, idx (B,N,k) i32 -> smooth (T)
torch::Tensor flow_smooth_fwd(torch::Tensor flows, torch::Tensor idx) {
  flow_smooth_check(flows, idx);
  const int64_t T = flows.size(0), B = flows.size(1), N = flows.size(2);
  const int64_t k = idx.size(2);
  const int nblk = flow_smooth_blocks((int)N);
  auto part = torch::empty({T, B * (int64_t)nblk}, flows.options());
  launch_flow_smooth_fwd(flows.data_ptr<float>(), idx.data_ptr<int>(),
                         part.data_ptr<float>(), (int)B, (int)N, (int)k, (int)T,
                         stream());
  return part.sum(1) / (double)(B * N * k);
}

torch::Tensor flow_smooth_bwd(torch::Tensor flows, torch::Tensor idx,
                              torch::Tensor offsets, torch::Tensor order_n,
                              torch::Tensor gout) {
  flow_smooth_check(flows, idx);
  check_i32(offsets, "offsets");
  check_i32(order_n, "order_n");
  check_f32(gout, "grad");
  const int64_t T = flows.size(0), B = flows.size(1), N = flows.size(2);
  const int64_t k = idx.size(2);
  TORCH_CHECK(offsets.numel() == B * (N + 1) && order_n.numel() == B * N * k &&
                  gout.numel() == T,
              "flow_smooth_bwd CSR / gradient shape mismatch");
  TORCH_CHECK(offsets.device() == flows.device() && order_n.device() == flows.device() &&
                  gout.device() == flows.device(),
              "flow_smooth_bwd inputs must share a device");
  auto dflow = torch::empty_like(flows);
  launch_flow_smooth_bwd(flows.data_ptr<float>(), idx.data_ptr<int>(),
                         offsets.data_ptr<int>(), order_n.data_ptr<int>(),
                         gout.data_ptr<float>(), dflow.data_ptr<float>(), (int)B,
                         (int)N, (int)k, (int)T, stream());
  return dflow;
}

// src (B,N,3), dst (B,N,3) f32, optional prior weights (B,N) f32 ->
// {R (B,3,3) f32, t (B,3) f32, residual (B,N) f32, ok (B) bool}: weighted
// Kabsch fit inside `iters` rounds of Cauchy reweighting, one launch, no
// host synchronisation
std::vector<torch::Tensor> rigid_fit(torch::Tensor src, torch::Tensor dst,
                                     c10::optional<torch::Tensor> weights,
                                     double thresh, int64_t iters) {
  check_f32(src, "src");
  check_f32(dst, "dst");
  TORCH_CHECK(src.dim() == 3 && src.size(2) == 3, "src must be (B,N,3)");
  TORCH_CHECK(dst.sizes() == src.sizes() && dst.device() == src.device(),
              "dst must match src in shape and device");
  const int64_t B = src.size(0), N = src.size(1);
  TORCH_CHECK(B >= 1 && N >= 1, "rigid_fit requires B, N >= 1");
  TORCH_CHECK(N < (1L << 30), "rigid_fit sizes exceed 32-bit point indexing");
  TORCH_CHECK(iters >= 0 && iters <= 64, "rigid_fit requires 0 <= iters <= 64");
  TORCH_CHECK(thresh > 0.0, "rigid_fit requires thresh > 0");
  const float* wp = nullptr;
  if (weights.has_value()) {
    const torch::Tensor& w = *weights;
    check_f32(w, "weights");
    TORCH_CHECK(w.dim() == 2 && w.size(0) == B && w.size(1) == N &&
                    w.device() == src.device(),
                "weights must be (B,N) on the device of src");
    wp = w.data_ptr<float>();
  }
  auto R = torch::empty({B, 3, 3}, src.options());
  auto t = torch::empty({B, 3}, src.options());
  auto res = torch::empty({B, N}, src.options());
  auto ok = torch::empty({B}, src.options().dtype(torch::kBool));
  launch_rigid_fit(src.data_ptr<float>(), dst.data_ptr<float>(), wp,
                   R.data_ptr<float>(), t.data_ptr<float>(),
                   res.data_ptr<float>(),
                   reinterpret_cast<unsigned char*>(ok.data_ptr<bool>()), (int)B,
                   (int)N, (float)thresh, (int)iters, stream());
  return {R, t, res, ok};
}

// rigid_fit once per segment: labels (B,N) i32 in [-1, M) (anything else
// counts as -1) -> {R (B,M,3,3), t (B,M,3), residual (B,N), ok (B,M) bool};
// one launch, grid (M, B), no host synchronisation
std::vector<torch::Tensor> segmented_rigid_fit(
    torch::Tensor src, torch::Tensor dst, torch::Tensor labels, int64_t M,
    c10::optional<torch::Tensor> weights, double thresh, int64_t iters) {
  check_f32(src, "src");
  check_f32(dst, "dst");
  TORCH_CHECK(src.dim() == 3 && src.size(2) == 3, "src must be (B,N,3)");
  TORCH_CHECK(dst.sizes() == src.sizes() && dst.device() == src.device(),
              "dst must match src in shape and device");
  const int64_t B = src.size(0), N = src.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1, "segmented_rigid_fit requires 1 <= B <= 65535, N >= 1");
  TORCH_CHECK(N < (1L << 30), "segmented_rigid_fit sizes exceed 32-bit point indexing");
  TORCH_CHECK(M >= 1 && M <= 65535, "segmented_rigid_fit requires 1 <= num_segments <= 65535");
  TORCH_CHECK(iters >= 0 && iters <= 64, "segmented_rigid_fit requires 0 <= iters <= 64");
  TORCH_CHECK(thresh > 0.0, "segmented_rigid_fit requires thresh > 0");
  TORCH_CHECK(labels.is_cuda() && labels.is_contiguous() &&
                  labels.scalar_type() == torch::kInt32 && labels.dim() == 2 &&
                  labels.size(0) == B && labels.size(1) == N &&
                  labels.device() == src.device(),
              "labels must be contiguous int32 (B,N) on the device of src");
  const float* wp = nullptr;
  if (weights.has_value()) {
    const torch::Tensor& w = *weights;
    check_f32(w, "weights");
    TORCH_CHECK(w.dim() == 2 && w.size(0) == B && w.size(1) == N &&
                    w.device() == src.device(),
                "weights must be (B,N) on the device of src");
    wp = w.data_ptr<float>();
  }
  auto R = torch::empty({B, M, 3, 3}, src.options());
  auto t = torch::empty({B, M, 3}, src.options());
  auto res = torch::empty({B, N}, src.options());
  auto ok = torch::empty({B, M}, src.options().dtype(torch::kBool));
  launch_segmented_rigid_fit(
      src.data_ptr<float>(), dst.data_ptr<float>(), wp, labels.data_ptr<int>(),
      R.data_ptr<float>(), t.data_ptr<float>(), res.data_ptr<float>(),
      reinterpret_cast<unsigned char*>(ok.data_ptr<bool>()), (int)B, (int)N,
      (int)M, (float)thresh, (int)iters, stream());
  return {R, t, res, ok};
}

// xyz, flow (B,N,3) f32, mask (B,N) bool -> {labels (B,N) i32, count (B,M)
// i32, num_objects (B) i32}: connected components of the radius graph in
// space and flow, ranked by size; five launches, no host synchronisation.
// The workspace is allocated here and initialised by the first kernel.
std::vector<torch::Tensor> cluster_points(torch::Tensor xyz, torch::Tensor flow,
                                          torch::Tensor mask, double eps,
                                          double flow_eps, int64_t min_points,
                                          int64_t M) {
  check_f32(xyz, "xyz");
  check_f32(flow, "flow");
  TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "xyz must be (B,N,3)");
  TORCH_CHECK(flow.sizes() == xyz.sizes() && flow.device() == xyz.device(),
              "flow must match xyz in shape and device");
  const int64_t B = xyz.size(0), N = xyz.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1, "cluster_points requires 1 <= B <= 65535, N >= 1");
  // the link grid has nblk (nblk + 1) / 2 workgroups in grid.x
  TORCH_CHECK(N <= (1L << 22), "cluster_points supports at most 2^22 points per cloud");
  TORCH_CHECK(M >= 1 && M <= 256, "cluster_points requires 1 <= max_objects <= 256");
  TORCH_CHECK(min_points >= 3, "cluster_points requires min_points >= 3");
  TORCH_CHECK(eps >= 0.0 && flow_eps >= 0.0, "cluster_points requires eps, flow_eps >= 0");
  TORCH_CHECK(mask.is_cuda() && mask.is_contiguous() &&
                  mask.scalar_type() == torch::kBool && mask.dim() == 2 &&
                  mask.size(0) == B && mask.size(1) == N &&
                  mask.device() == xyz.device(),
              "mask must be contiguous bool (B,N) on the device of xyz");
  auto iopt = xyz.options().dtype(torch::kInt32);
  auto ws = torch::empty({5, B, N}, iopt);
  auto status = torch::empty({B}, iopt);
  auto labels = torch::empty({B, N}, iopt);
  auto count = torch::empty({B, M}, iopt);
  auto nobj = torch::empty({B}, iopt);
  launch_cluster_points(
      xyz.data_ptr<float>(), flow.data_ptr<float>(),
      reinterpret_cast<const unsigned char*>(mask.data_ptr<bool>()),
      ws.data_ptr<int>(), status.data_ptr<int>(), labels.data_ptr<int>(),
      count.data_ptr<int>(), nobj.data_ptr<int>(), (int)B, (int)N, (int)M,
      (float)eps, (float)flow_eps, (int)std::min<int64_t>(min_points, INT32_MAX),
      stream());
  return {labels, count, nobj};
}

// Ground-plane fit (csrc/plane_fit.hip).  xyz (B,N,3) f32, optional mask (B,N)
// bool.  up / cos2 / thresh2 arrive already rounded to fp32 by the caller so
// every backend tests against the same numbers.  refine_iters < 0 stops after
// the scores: {idx (B,H,3) i32, count (B,H) i32}.  Otherwise {normal (B,3),
// offset (B), height (B,N), ground (B,N) bool, inlier (B,N) bool, count (B)
// i32, best (B) i32, rounds (B) i32, ok (B) bool}.  Four launches, no host
// synchronisation.
std::vector<torch::Tensor> plane_fit(torch::Tensor xyz,
                                     c10::optional<torch::Tensor> mask,
                                     double thresh, double thresh2, double cos2,
                                     double upx, double upy, double upz,
                                     int64_t H, int64_t refine_iters,
                                     int64_t seed) {
  check_f32(xyz, "xyz");
  TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "xyz must be (B,N,3)");
  const int64_t B = xyz.size(0), N = xyz.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1, "plane_fit requires 1 <= B <= 65535, N >= 1");
  TORCH_CHECK(N < (1L << 30), "plane_fit sizes exceed 32-bit point indexing");
  TORCH_CHECK(H >= 1 && H <= 4096, "plane_fit requires 1 <= hypotheses <= 4096");
  TORCH_CHECK(refine_iters <= 16, "plane_fit requires refine_iters <= 16");
  TORCH_CHECK(thresh > 0.0 && thresh2 > 0.0, "plane_fit requires thresh > 0");
  const unsigned char* mp = nullptr;
  if (mask.has_value()) {
    const torch::Tensor& m = *mask;
    TORCH_CHECK(m.is_cuda() && m.is_contiguous() &&
                    m.scalar_type() == torch::kBool && m.dim() == 2 &&
                    m.size(0) == B && m.size(1) == N &&
                    m.device() == xyz.device(),
                "mask must be contiguous bool (B,N) on the device of xyz");
    mp = reinterpret_cast<const unsigned char*>(m.data_ptr<bool>());
  }
  auto iopt = xyz.options().dtype(torch::kInt32);
  auto bopt = xyz.options().dtype(torch::kBool);
  auto idx = torch::empty({B, H, 3}, iopt);
  auto cnt = torch::empty({B, H}, iopt);
  auto rec = torch::empty({B, H, 8}, xyz.options());
  launch_plane_hypotheses(xyz.data_ptr<float>(), mp, idx.data_ptr<int>(),
                          rec.data_ptr<float>(), cnt.data_ptr<int>(), (int)B,
                          (int)N, (int)H, (unsigned)(seed & 0xffffffffL),
                          (float)upx, (float)upy, (float)upz, (float)cos2,
                          (float)thresh2, stream());
  if (refine_iters < 0) return {idx, cnt};
  auto normal = torch::empty({B, 3}, xyz.options());
  auto offset = torch::empty({B}, xyz.options());
  auto height = torch::empty({B, N}, xyz.options());
  auto ground = torch::empty({B, N}, bopt);
  auto inlier = torch::empty({B, N}, bopt);
  auto count = torch::empty({B}, iopt);
  auto best = torch::empty({B}, iopt);
  auto rounds = torch::empty({B}, iopt);
  auto ok = torch::empty({B}, bopt);
  auto plane64 = torch::empty({B, 8}, xyz.options().dtype(torch::kFloat64));
  launch_plane_refine(
      xyz.data_ptr<float>(), mp, rec.data_ptr<float>(), cnt.data_ptr<int>(),
      normal.data_ptr<float>(), offset.data_ptr<float>(),
      height.data_ptr<float>(),
      reinterpret_cast<unsigned char*>(ground.data_ptr<bool>()),
      reinterpret_cast<unsigned char*>(inlier.data_ptr<bool>()),
      count.data_ptr<int>(), best.data_ptr<int>(), rounds.data_ptr<int>(),
      reinterpret_cast<unsigned char*>(ok.data_ptr<bool>()),
      plane64.data_ptr<double>(), (int)B, (int)N, (int)H, (int)refine_iters,
      thresh, (float)upx, (float)upy, (float)upz, (float)cos2, stream());
  return {normal, offset, height, ground, inlier, count, best, rounds, ok};
}

// Voxel-stratified sampling (csrc/voxel_sample.hip).  xyz (B,N,3) f32,
// optional mask (B,N) bool, inv = fp32(1 / voxel) from the caller so every
// backend multiplies by the same number -> {idx (B,m) i64, count (B) i32,
// rank (B,N) i32, occupied (B,levels) i32}.  10 + levels launches, no host
// synchronisation.  The workspaces are torch allocations of this call; the
// first kernel initialises every word that is read before it is written.
std::vector<torch::Tensor> voxel_sample(torch::Tensor xyz,
                                        c10::optional<torch::Tensor> mask,
                                        int64_t m, double inv, int64_t levels,
                                        int64_t seed) {
  check_f32(xyz, "xyz");
  TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "xyz must be (B,N,3)");
  const int64_t B = xyz.size(0), N = xyz.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1, "voxel_sample requires 1 <= B <= 65535, N >= 1");
  TORCH_CHECK(N < (1L << 27), "voxel_sample requires N < 2^27");
  TORCH_CHECK(m >= 1, "voxel_sample requires m >= 1");
  TORCH_CHECK(levels >= 1 && levels <= 16, "voxel_sample requires 1 <= levels <= 16");
  TORCH_CHECK(inv > 0.0 && std::isfinite(inv), "voxel_sample requires a finite 1 / voxel > 0");
  const unsigned char* mp = nullptr;
  if (mask.has_value()) {
    const torch::Tensor& k = *mask;
    TORCH_CHECK(k.is_cuda() && k.is_contiguous() &&
                    k.scalar_type() == torch::kBool && k.dim() == 2 &&
                    k.size(0) == B && k.size(1) == N &&
                    k.device() == xyz.device(),
                "mask must be contiguous bool (B,N) on the device of xyz");
    mp = reinterpret_cast<const unsigned char*>(k.data_ptr<bool>());
  }
  int64_t T = 2;  // slots per table and cloud: a power of two >= 2 N
  while (T < 2 * N) T <<= 1;
  const int64_t nblk = (N + voxel_sample_block() - 1) / voxel_sample_block();
  auto iopt = xyz.options().dtype(torch::kInt32);
  auto lopt = xyz.options().dtype(torch::kInt64);
  auto tab = torch::empty({6, B, T}, lopt);
  auto key0 = torch::empty({B, N}, lopt);
  auto slots = torch::empty({2, B, N}, iopt);
  auto sel = torch::empty({B, N}, xyz.options().dtype(torch::kUInt8));
  auto bsum = torch::empty({B, nblk}, iopt);
  auto meta = torch::empty({B, (int64_t)voxel_sample_meta()}, iopt);
  auto idx = torch::empty({B, m}, lopt);
  auto count = torch::empty({B}, iopt);
  auto rank = torch::empty({B, N}, iopt);
  auto occ = torch::empty({B, levels}, iopt);
  launch_voxel_sample(
      xyz.data_ptr<float>(), mp,
      reinterpret_cast<unsigned long long*>(tab.data_ptr<int64_t>()),
      reinterpret_cast<unsigned long long*>(key0.data_ptr<int64_t>()),
      slots.data_ptr<int>(), sel.data_ptr<uint8_t>(), bsum.data_ptr<int>(),
      meta.data_ptr<int>(), reinterpret_cast<long*>(idx.data_ptr<int64_t>()),
      count.data_ptr<int>(), rank.data_ptr<int>(), occ.data_ptr<int>(), (int)B,
      (int)N, (int)T, (long)m, (int)levels, (float)inv,
      (unsigned)(seed & 0xffffffffL), stream());
  return {idx, count, rank, occ};
}

// Noise filter (csrc/noise_filter.hip).  xyz (B,N,3) f32, optional mask (B,N)
// bool, inv = fp32(1 / radius) and r2 = fp32(radius)^2 from the caller so every
// backend computes with the same numbers -> {keep (B,N) bool, count (B,N) i32,
// mean_dist (B,N) f32, stats (B,3) f64 = mean, std, threshold, ok (B) bool}.
// 9 launches, no host synchronisation.  The workspaces are torch allocations
// of this call; every word is written before it is read.
std::vector<torch::Tensor> noise_filter(torch::Tensor xyz,
                                        c10::optional<torch::Tensor> mask,
                                        double inv, double r2, int64_t k,
                                        int64_t min_neighbors,
                                        double std_ratio) {
  check_f32(xyz, "xyz");
  TORCH_CHECK(xyz.dim() == 3 && xyz.size(2) == 3, "xyz must be (B,N,3)");
  const int64_t B = xyz.size(0), N = xyz.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && N >= 1, "noise_filter requires 1 <= B <= 65535, N >= 1");
  TORCH_CHECK(N < (1L << 27), "noise_filter requires N < 2^27");
  TORCH_CHECK(k >= 0 && k <= 16, "noise_filter requires 0 <= k <= 16");
  TORCH_CHECK(min_neighbors >= 0, "noise_filter requires min_neighbors >= 0");
  TORCH_CHECK(inv > 0.0 && std::isfinite(inv) && r2 >= 0.0, "noise_filter requires a finite 1 / radius > 0");
  TORCH_CHECK(std_ratio >= 0.0, "noise_filter requires std_ratio >= 0");
  const unsigned char* mp = nullptr;
  if (mask.has_value()) {
    const torch::Tensor& q = *mask;
    TORCH_CHECK(q.is_cuda() && q.is_contiguous() &&
                    q.scalar_type() == torch::kBool && q.dim() == 2 &&
                    q.size(0) == B && q.size(1) == N &&
                    q.device() == xyz.device(),
                "mask must be contiguous bool (B,N) on the device of xyz");
    mp = reinterpret_cast<const unsigned char*>(q.data_ptr<bool>());
  }
  int64_t T = 2;  // slots per cloud: a power of two >= 2 N
  while (T < 2 * N) T <<= 1;
  const int64_t blk = noise_filter_block();
  const int64_t nblk = (N + blk - 1) / blk, nrun = (T + blk - 1) / blk;
  auto iopt = xyz.options().dtype(torch::kInt32);
  auto bopt = xyz.options().dtype(torch::kBool);
  auto dopt = xyz.options().dtype(torch::kFloat64);
  auto keys = torch::empty({B, T}, xyz.options().dtype(torch::kInt64));
  auto cells = torch::empty({2, B, T}, iopt);
  auto slot = torch::empty({B, N}, iopt);
  auto sorted = torch::empty({B, N, 4}, xyz.options());
  auto bsum = torch::empty({B, nrun}, iopt);
  auto meta = torch::empty({2, B}, iopt);
  auto part = torch::empty({B, 3, nblk}, dopt);
  auto keep = torch::empty({B, N}, bopt);
  auto count = torch::empty({B, N}, iopt);
  auto md = torch::empty({B, N}, xyz.options());
  auto stats = torch::empty({B, 3}, dopt);
  auto ok = torch::empty({B}, bopt);
  launch_noise_filter(
      xyz.data_ptr<float>(), mp,
      reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>()),
      cells.data_ptr<int>(), slot.data_ptr<int>(), sorted.data_ptr<float>(),
      bsum.data_ptr<int>(), meta.data_ptr<int>(), part.data_ptr<double>(),
      reinterpret_cast<unsigned char*>(keep.data_ptr<bool>()),
      count.data_ptr<int>(), md.data_ptr<float>(), stats.data_ptr<double>(),
      reinterpret_cast<unsigned char*>(ok.data_ptr<bool>()), (int)B, (int)N,
      (int)T, (float)inv, (float)r2, (int)k,
      (int)std::min<int64_t>(min_neighbors, INT32_MAX), std_ratio, stream());
  return {keep, count, md, stats, ok};
}

// Grid search and ICP (csrc/grid_nn.hip).
namespace {

const unsigned char* gn_mask(const c10::optional<torch::Tensor>& mask,
                             const torch::Tensor& like, const char* name) {
  if (!mask.has_value()) return nullptr;
  const torch::Tensor& q = *mask;
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() &&
                  q.scalar_type() == torch::kBool && q.dim() == 2 &&
                  q.size(0) == like.size(0) && q.size(1) == like.size(1) &&
                  q.device() == like.device(),
              name, " must be contiguous bool (B,N) on the device of its cloud");
  return reinterpret_cast<const unsigned char*>(q.data_ptr<bool>());
}

const float* gn_pose(const c10::optional<torch::Tensor>& v,
                     const torch::Tensor& like, bool rot, const char* name) {
  if (!v.has_value()) return nullptr;
  const torch::Tensor& q = *v;
  check_f32(q, name);
  TORCH_CHECK(q.device() == like.device() && q.size(0) == like.size(0) &&
                  (rot ? (q.dim() == 3 && q.size(1) == 3 && q.size(2) == 3)
                       : (q.dim() == 2 && q.size(1) == 3)),
              name, rot ? " must be (B,3,3)" : " must be (B,3)",
              " on the device of the query");
  return q.data_ptr<float>();
}

// The workspaces of one grid over `support`: torch allocations of the call;
// every word is written before it is read.
struct GridNN {
  torch::Tensor keys, cells, slot, sorted, bsum;
  int64_t T;
  GridNN(const torch::Tensor& support) {
    const int64_t B = support.size(0), M = support.size(1);
    T = 2;  // slots per cloud: a power of two >= 2 M
    while (T < 2 * M) T <<= 1;
    const int64_t blk = grid_nn_block(), nrun = (T + blk - 1) / blk;
    auto iopt = support.options().dtype(torch::kInt32);
    keys = torch::empty({B, T}, support.options().dtype(torch::kInt64));
    cells = torch::empty({2, B, T}, iopt);
    slot = torch::empty({B, M}, iopt);
    sorted = torch::empty({B, M, 4}, support.options());
    bsum = torch::empty({B, nrun}, iopt);
  }
  unsigned long long* k() {
    return reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>());
  }
};

void gn_check(const torch::Tensor& query, const torch::Tensor& support,
              double inv, double r2, const char* op) {
  check_f32(query, "query");
  check_f32(support, "support");
  TORCH_CHECK(query.dim() == 3 && query.size(2) == 3, op, ": query must be (B,N,3)");
  TORCH_CHECK(support.dim() == 3 && support.size(2) == 3 &&
                  support.size(0) == query.size(0) &&
                  support.device() == query.device(),
              op, ": support must be (B,M,3) on the device of the query");
  const int64_t B = query.size(0), Nq = query.size(1), M = support.size(1);
  TORCH_CHECK(B >= 1 && B <= 65535 && Nq >= 1 && M >= 1, op,
              " requires 1 <= B <= 65535 and at least one point per cloud");
  TORCH_CHECK(Nq < (1L << 27) && M < (1L << 27), op, " requires N, M < 2^27");
  TORCH_CHECK(inv > 0.0 && std::isfinite(inv) && r2 >= 0.0, op,
              " requires a finite 1 / radius > 0");
}

}  // namespace

// query (B,Nq,3), support (B,M,3) f32, optional masks, optional R (B,3,3) and
// t (B,3) read on the device, inv = fp32(1 / radius) and r2 = fp32(radius)^2
// from the caller -> {idx (B,Nq) i32, d2 (B,Nq) f32, ok (B) bool}.  6 launches,
// no host synchronisation.
std::vector<torch::Tensor> nearest_in_radius(
    torch::Tensor query, torch::Tensor support,
    c10::optional<torch::Tensor> query_mask,
    c10::optional<torch::Tensor> support_mask, c10::optional<torch::Tensor> R,
    c10::optional<torch::Tensor> t, double inv, double r2) {
  gn_check(query, support, inv, r2, "nearest_in_radius");
  TORCH_CHECK(R.has_value() == t.has_value(), "nearest_in_radius: R and t go together");
  const int64_t B = query.size(0), Nq = query.size(1), M = support.size(1);
  const unsigned char* qm = gn_mask(query_mask, query, "query_mask");
  const unsigned char* sm = gn_mask(support_mask, support, "support_mask");
  const float* Rp = gn_pose(R, query, true, "R");
  const float* tp = gn_pose(t, query, false, "t");
  GridNN g(support);
  auto iopt = query.options().dtype(torch::kInt32);
  auto status = torch::empty({B}, iopt);
  auto idx = torch::empty({B, Nq}, iopt);
  auto d2 = torch::empty({B, Nq}, query.options());
  auto ok = torch::empty({B}, query.options().dtype(torch::kBool));
  unsigned char* okp = reinterpret_cast<unsigned char*>(ok.data_ptr<bool>());
  launch_grid_nn_build(support.data_ptr<float>(), sm, g.k(), g.cells.data_ptr<int>(),
                       g.slot.data_ptr<int>(), g.sorted.data_ptr<float>(),
                       g.bsum.data_ptr<int>(), status.data_ptr<int>(), B, okp,
                       nullptr, nullptr, nullptr, nullptr, (int)B, (int)M,
                       (int)g.T, (float)inv, stream());
  launch_grid_nn_query(query.data_ptr<float>(), qm, Rp, tp, g.k(),
                       g.cells.data_ptr<int>(), g.sorted.data_ptr<float>(),
                       g.bsum.data_ptr<int>(), status.data_ptr<int>(), okp,
                       idx.data_ptr<int>(), d2.data_ptr<float>(), nullptr, nullptr,
                       nullptr, (int)B, (int)Nq, (int)M, (int)g.T, (float)inv,
                       (float)r2, 1.0f, stream());
  return {idx, d2, ok};
}

// Point-to-point ICP of src (B,N,3) against dst (B,M,3): the grid over dst
// once, then per round search / rigid_fit (iters = 0) / commit, and a closing
// search: 5 + 3 * iters + 1 launches, no host synchronisation.  th2 =
// fp32(thresh)^2 from the caller.  -> {R (B,3,3), t (B,3), idx (B,N) i32, d2
// (B,N), matched (B) i32, rounds (B) i32, ok (B) bool}.
std::vector<torch::Tensor> icp_refine(
    torch::Tensor src, torch::Tensor dst, c10::optional<torch::Tensor> src_mask,
    c10::optional<torch::Tensor> dst_mask, c10::optional<torch::Tensor> R0,
    c10::optional<torch::Tensor> t0, double inv, double r2, double th2,
    int64_t iters) {
  gn_check(src, dst, inv, r2, "icp_refine");
  TORCH_CHECK(iters >= 0 && iters <= 64, "icp_refine requires 0 <= iters <= 64");
  TORCH_CHECK(th2 > 0.0 && std::isfinite(th2), "icp_refine requires a finite thresh^2 > 0");
  const int64_t B = src.size(0), N = src.size(1), M = dst.size(1);
  const unsigned char* sm = gn_mask(src_mask, src, "src_mask");
  const unsigned char* dm = gn_mask(dst_mask, dst, "dst_mask");
  const float* R0p = gn_pose(R0, src, true, "R0");
  const float* t0p = gn_pose(t0, src, false, "t0");
  GridNN g(dst);
  auto iopt = src.options().dtype(torch::kInt32);
  auto bopt = src.options().dtype(torch::kBool);
  // rows: status, stopped, rounds, then one match counter per search
  auto state = torch::empty({3 + iters + 1, B}, iopt);
  int* st = state.data_ptr<int>();
  auto R = torch::empty({B, 3, 3}, src.options());
  auto t = torch::empty({B, 3}, src.options());
  auto Rfit = torch::empty({B, 3, 3}, src.options());
  auto tfit = torch::empty({B, 3}, src.options());
  auto res = torch::empty({B, N}, src.options());
  auto fit_ok = torch::empty({B}, bopt);
  auto mdst = torch::empty({B, N, 3}, src.options());
  auto wgt = torch::empty({B, N}, src.options());
  auto idx = torch::empty({B, N}, iopt);
  auto d2 = torch::empty({B, N}, src.options());
  auto ok = torch::empty({B}, bopt);
  unsigned char* okp = reinterpret_cast<unsigned char*>(ok.data_ptr<bool>());
  unsigned char* fop = reinterpret_cast<unsigned char*>(fit_ok.data_ptr<bool>());
  launch_grid_nn_build(dst.data_ptr<float>(), dm, g.k(), g.cells.data_ptr<int>(),
                       g.slot.data_ptr<int>(), g.sorted.data_ptr<float>(),
                       g.bsum.data_ptr<int>(), st, (3 + iters + 1) * B, okp,
                       R.data_ptr<float>(), t.data_ptr<float>(), R0p, t0p, (int)B,
                       (int)M, (int)g.T, (float)inv, stream());
  for (int64_t k = 0; k <= iters; ++k) {
    launch_grid_nn_query(src.data_ptr<float>(), sm, R.data_ptr<float>(),
                         t.data_ptr<float>(), g.k(), g.cells.data_ptr<int>(),
                         g.sorted.data_ptr<float>(), g.bsum.data_ptr<int>(), st, okp,
                         idx.data_ptr<int>(), d2.data_ptr<float>(),
                         mdst.data_ptr<float>(), wgt.data_ptr<float>(),
                         st + (3 + k) * B, (int)B, (int)N, (int)M, (int)g.T,
                         (float)inv, (float)r2, (float)th2, stream());
    if (k == iters) break;
    launch_rigid_fit(src.data_ptr<float>(), mdst.data_ptr<float>(),
                     wgt.data_ptr<float>(), Rfit.data_ptr<float>(),
                     tfit.data_ptr<float>(), res.data_ptr<float>(), fop, (int)B,
                     (int)N, 1.0f, 0, stream());
    launch_icp_commit(st + (3 + k) * B, fop, Rfit.data_ptr<float>(),
                      tfit.data_ptr<float>(), R.data_ptr<float>(),
                      t.data_ptr<float>(), st + B, st + 2 * B, okp, (int)B,
                      stream());
  }
  return {R, t, idx, d2, state[3 + iters], state[2], ok};
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("nearest_in_radius", &nearest_in_radius);
  m.def("icp_refine", &icp_refine);
  m.def("noise_filter", &noise_filter);
  m.attr("NOISE_FILTER_BLOCK") = noise_filter_block();
  m.attr("NOISE_FILTER_SCAN") = noise_filter_scan();
  m.def("voxel_sample", &voxel_sample);
  m.attr("VOXEL_SAMPLE_BLOCK") = voxel_sample_block();
  m.attr("VOXEL_SAMPLE_SCAN") = voxel_sample_scan();
  m.def("plane_fit", &plane_fit);
  m.attr("PLANE_SCORE_TILE") = plane_score_tile();
  m.attr("PLANE_SCORE_BLOCK") = plane_score_block();
  m.attr("PLANE_REFINE_BLOCK") = plane_refine_block();
  m.def("rigid_fit", &rigid_fit);
  m.attr("RIGID_FIT_REG_POINTS") = rigid_fit_reg_points();
  m.def("segmented_rigid_fit", &segmented_rigid_fit);
  m.attr("SEGMENTED_FIT_CAPACITY") = segmented_fit_capacity();
  m.def("cluster_points", &cluster_points);
  m.attr("CLUSTER_TILE") = cluster_tile();
  m.def("chamfer_fwd", &chamfer_fwd);
  m.def("chamfer_nn_fwd", &chamfer_nn_fwd);
  m.def("chamfer_bwd", &chamfer_bwd);
  m.attr("CHAMFER_TILE") = chamfer_tile_pts();
  m.def("flow_smooth_fwd", &flow_smooth_fwd);
  m.def("flow_smooth_bwd", &flow_smooth_bwd);
  m.def("topk_rows", &topk_rows);
  m.def("corr_topk", &corr_topk);
  m.def("corr_grad_expand", &corr_grad_expand);
  m.def("corr_gather_xyz", &corr_gather_xyz);
  m.def("seq_loss_fwd", &seq_loss_fwd);
  m.def("seq_loss_bwd", &seq_loss_bwd);
  m.def("gru_zr_fwd", &gru_zr_fwd);
  m.def("gru_zr_bwd", &gru_zr_bwd);
  m.def("gru_q_fwd", &gru_q_fwd);
  m.def("gru_q_bwd", &gru_q_bwd);
  m.def("pv_corr_fused_fwd", &pv_corr_fused_fwd);
  m.def("pv_corr_fused_bwd", &pv_corr_fused_bwd);
  m.def("pw_wgrad", &pw_wgrad, pybind11::arg("dy"), pybind11::arg("x"), pybind11::arg("schunks") = 0, pybind11::arg("with_bias") = false);
  m.def("pw_wgrad_batched", &pw_wgrad_batched);
  m.def("pw_fwd", &pw_fwd, pybind11::arg("ws"), pybind11::arg("xs"),
        pybind11::arg("bias"), pybind11::arg("addend"), pybind11::arg("act"),
        pybind11::arg("point_major") = false);
  m.def("pw_bwd", &pw_bwd, pybind11::arg("dy"), pybind11::arg("y"),
        pybind11::arg("ws"), pybind11::arg("want"), pybind11::arg("act"),
        pybind11::arg("point_major") = false,
        pybind11::arg("slab") = pybind11::none(), pybind11::arg("r0") = 0);
  m.def("batched_transpose", &batched_transpose);
  m.def("group_norm_act_fwd", &group_norm_act_fwd);
  m.def("group_norm_act_bwd", &group_norm_act_bwd);
  m.def("group_norm_act_maxpool_fwd", &group_norm_act_maxpool_fwd);
  m.def("group_norm_act_maxpool_bwd", &group_norm_act_maxpool_bwd);
  m.def("edge_gnmp_fwd", &edge_gnmp_fwd, pybind11::arg("wg"),
        pybind11::arg("idx"), pybind11::arg("G"), pybind11::arg("weight"),
        pybind11::arg("bias"), pybind11::arg("eps"), pybind11::arg("act"),
        pybind11::arg("slope"), pybind11::arg("slope_t"),
        pybind11::arg("channel_major_out") = false,
        pybind11::arg("classic") = false);
  m.def("edge_gnmp_bwd", &edge_gnmp_bwd, pybind11::arg("dy"),
        pybind11::arg("wg"), pybind11::arg("idx"), pybind11::arg("am"),
        pybind11::arg("vsel"), pybind11::arg("vsum"),
        pybind11::arg("offsets"), pybind11::arg("order_n"),
        pybind11::arg("order_j"), pybind11::arg("mean"),
        pybind11::arg("rstd"), pybind11::arg("G"), pybind11::arg("weight"),
        pybind11::arg("bias"), pybind11::arg("act"), pybind11::arg("slope"),
        pybind11::arg("slope_t"), pybind11::arg("wtarget"),
        pybind11::arg("btarget"), pybind11::arg("starget"),
        pybind11::arg("classic") = false);
  m.def("morton_keys", &morton_keys);
  m.def("multi_cast_bf16", &multi_cast_bf16);
  m.def("knn_gnmp_fwd", &knn_gnmp_fwd, pybind11::arg("raw"),
        pybind11::arg("W"), pybind11::arg("cb"), pybind11::arg("G"),
        pybind11::arg("gamma"), pybind11::arg("beta"), pybind11::arg("eps"),
        pybind11::arg("slope_t"), pybind11::arg("out_bf16"),
        pybind11::arg("channel_major_out") = false);
  m.def("knn_gnmp_bwd", &knn_gnmp_bwd, pybind11::arg("dy"),
        pybind11::arg("raw"), pybind11::arg("W"), pybind11::arg("cb"),
        pybind11::arg("am"), pybind11::arg("vsel"), pybind11::arg("mean"),
        pybind11::arg("rstd"), pybind11::arg("G"), pybind11::arg("gamma"),
        pybind11::arg("beta"), pybind11::arg("slope_t"), pybind11::arg("eps"),
        pybind11::arg("dy_channel_major") = false,
        pybind11::arg("wtarget") = pybind11::none(),
        pybind11::arg("cbtarget") = pybind11::none(),
        pybind11::arg("gtarget") = pybind11::none(),
        pybind11::arg("btarget") = pybind11::none(),
        pybind11::arg("starget") = pybind11::none());
  m.def("knn_graph", &knn_graph, "fused kNN graph (CDNA4)");
  m.def("knn_csr", &knn_csr, "inverse kNN adjacency as CSR (counting sort)");
  m.def("knn_interp_fwd", &knn_interp_fwd);
  m.attr("KNN_INTERP_TILE") = knn_interp_tile_pts();
  m.def("gather_edge_concat_fwd", &gather_edge_concat_fwd);
  m.def("gather_edge_concat_bwd", &gather_edge_concat_bwd);
  m.def("gather_edge_bwd_csr", &gather_edge_bwd_csr);
  m.def("voxel_corr_fwd", &voxel_corr_fwd);
  m.def("voxel_corr_bwd", &voxel_corr_bwd);
  m.def("knn_corr_fwd", &knn_corr_fwd);
  m.def("knn_corr_bwd", &knn_corr_bwd);
}
