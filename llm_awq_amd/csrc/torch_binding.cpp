// Python module `awq_inference_engine` for PyTorch-ROCm: the reference's two hot-path exports
//     gemv_forward_cuda_new(in_feats, kernel, scaling_factors, zeros, m, n, k, group_size) -> Tensor
//     gemm_forward_cuda_new(in_feats, kernel, scales, zeros) -> Tensor
// (awq/kernels/csrc/pybind.cpp:22-23; gemv_cuda.cu:245-338; gemm_cuda.cu:1126-1236) re-implemented as a
// thin shim over the C ABI in include/awq_cdna4.h.  Same names, argument meaning, output
// allocation and error behaviour (RuntimeError); plus what the reference lacks: device guard,
// launch on the CURRENT stream, contiguity / shape checks.
// Torch is plumbing here (tensor memory, streams); all compute lives behind the C ABI.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/extension.h>

#include <cstdlib>
#include <mutex>
#include <tuple>
#include <stdexcept>
#include <string>
#include <unordered_map>

#include "../../include/awq_cdna4.h"

namespace {

int dtype_code(const torch::Tensor& t) {
  if (t.scalar_type() == at::kHalf) return AWQ_F16;
  if (t.scalar_type() == at::kBFloat16) return AWQ_BF16;
  TORCH_CHECK(false, "awq_inference_engine: only float16 / bfloat16 activations are supported, got ", t.scalar_type());
}

void raise_on(int st) {
  if (st == AWQ_OK) return;
  std::string msg = awq_status_string(st);
  if (st == AWQ_ERR_LAUNCH) msg += std::string(" ") + awq_last_hip_error();
  if (st == AWQ_ERR_BATCH || st == AWQ_ERR_GROUP) throw std::runtime_error(msg + "\n");  // gemv_cuda.cu:329,334
  TORCH_CHECK(false, "awq_inference_engine: ", msg);
}

void check_inputs(const torch::Tensor& x, const torch::Tensor& kernel, const torch::Tensor& scales,
                  const torch::Tensor& zeros) {
  TORCH_CHECK(x.is_cuda() && kernel.is_cuda() && scales.is_cuda() && zeros.is_cuda(),
              "awq_inference_engine: all tensors must live on the GPU (this build has no CPU path)");
  TORCH_CHECK(scales.scalar_type() == x.scalar_type());  // gemv_cuda.cu:260 / gemm_cuda.cu:1145
  TORCH_CHECK(zeros.scalar_type() == x.scalar_type());   // gemv_cuda.cu:261 / gemm_cuda.cu:1146
  TORCH_CHECK(kernel.scalar_type() == at::kShort, "qweight must be int16 [N/4, K]");
  TORCH_CHECK(x.is_contiguous() && kernel.is_contiguous() && scales.is_contiguous() && zeros.is_contiguous(),
              "awq_inference_engine: tensors must be contiguous");
  TORCH_CHECK(kernel.device() == x.device() && scales.device() == x.device() && zeros.device() == x.device(),
              "awq_inference_engine: tensors must be on the same device");
}

// ---------------------------------------------------------------------------------------------------------------
// Lazy v2 -> cdna4 cache.  tinychat hands the extension RAW reference-layout buffers (fused_mlp.py:40-77 passes
// gate_proj_qweight etc. directly, make_quant_attn concatenates v2 buffers after load), so the drop-in entry points
// cannot assume the repacker ran.  The first call with a given (qweight, scales, zeros) triple repacks
// them once on the GPU (awq_repack_v2_to_cdna4 + awq_pack_sz_cdna4, tens of microseconds) and later calls run the
// cdna4 kernels.  An entry is tied to the IDENTITY of the three tensors (weak TensorImpl references, so a freed
// tensor whose address is re-used can never hit) and to their version counters (an in-place update re-packs).
// Cost: a second packed copy of the weights (N*K/2 + N*K/32 bytes).  AWQ_CDNA4_AUTOCACHE=0 disables it.  While the stream is
// being captured into a hipGraph nothing is built (no allocations inside a capture): entries made by a warm-up call are used.
// ---------------------------------------------------------------------------------------------------------------
// One entry per qweight tensor: the permuted weights (the expensive part: N*K/2 bytes) are tied to the qweight's identity and
// version ONLY.  The packed scale buffers (3 % of that) hang off the entry in two slots keyed by the (scales, zeros) pair they
// were built from: tinychat's QuantLlamaMLP passes the module's scaled_zeros on its decode branch and a FRESH temporary
// (`scaled_zeros - 8 * scales`, fused_mlp.py:69,76) on every prefill call -- the temporary re-packs 1-2 MB of scales into the
// least recently used slot, never the weights, and the decode pair keeps hitting its own slot.
inline uint32_t tensor_version(const torch::Tensor& t) { return t.is_inference() ? 0u : (uint32_t)t._version(); }
struct SzSlot {
  c10::weak_intrusive_ptr<c10::TensorImpl> s, z;
  uint32_t vs = 0, vz = 0;
  at::Tensor szp, szh;  // sz_packed (T) and sz_half (decode; undefined when the layer's scales are not f16-exact)
  uint64_t stamp = 0;
  hipEvent_t built = nullptr;  // recorded behind the pack kernels; a hit from another stream waits for it until it has completed
  hipStream_t build_stream = nullptr;
  bool settled = false;
  bool expired() const { return !szp.defined() || s.expired() || z.expired(); }
  SzSlot() : s(c10::weak_intrusive_ptr<c10::TensorImpl>(c10::intrusive_ptr<c10::TensorImpl>())), z(s) {}
};
struct CacheEntry {
  c10::weak_intrusive_ptr<c10::TensorImpl> w;
  uint32_t vw;
  at::Tensor c4;
  SzSlot slot[2];
  hipEvent_t built = nullptr;  // recorded on the building stream; other streams wait for it until it has completed
  hipStream_t build_stream = nullptr;
  bool settled = false;
  // AWQ_CDNA4_INPLACE=1: the caller's qweight storage is converted where it lies (no second copy).  The entry does NOT own that storage -- a cache must
  // never extend the lifetime of the model's weights (`del model` has to give the memory back) -- it keeps a WEAK reference to it, the
  // view's geometry, and the version counter the module's tensor shares with its `.detach()` / `.data` / view aliases
  bool inplace = false;
  c10::weak_intrusive_ptr<c10::StorageImpl> ws{c10::intrusive_ptr<c10::StorageImpl>()};
  int64_t ws_offset = 0, ws_n4 = 0, ws_k = 0;
  c10::Device ws_dev{c10::DeviceType::CPU};
  bool has_vc = false;
  c10::VariableVersion vc{c10::VariableVersion::DISABLED};
  uint32_t vc4 = 0;  // the counter's value at conversion: a later value means the caller wrote fresh v2 bytes over the converted ones (copy_, load_state_dict)
  bool inplace_alive() const { return inplace && !ws.expired(); }
  // the converted bytes are still what the cache put there (false: storage gone, or overwritten since -- nothing to restore, nothing to follow)
  bool inplace_intact() const { return inplace_alive() && (!has_vc || (uint32_t)vc.current_version() == vc4); }
  bool holds(const torch::Tensor& t) const {  // is `t` a tensor over the converted storage?
    auto l = ws.lock();
    return l && l.get() == t.storage().unsafeGetStorageImpl();
  }
  // a tensor over the converted bytes (keeps the storage alive for the call); undefined if the storage is gone
  at::Tensor inplace_tensor() const {
    auto l = ws.lock();
    if (!l) return at::Tensor();
    at::Tensor t = at::empty({0}, at::TensorOptions().dtype(at::kShort).device(ws_dev));
    t.set_(c10::Storage(std::move(l)), ws_offset, {ws_n4, ws_k}, {ws_k, 1});
    return t;
  }
  explicit CacheEntry(const torch::Tensor& tw) : w(tw.getIntrusivePtr()), vw(tensor_version(tw)) {}
};
std::mutex g_cache_mu;
std::unordered_map<const void*, CacheEntry> g_cache;
int g_cache_enabled = -1, g_cache_inplace = -1;
int64_t g_cache_hits = 0, g_cache_builds = 0, g_cache_sz_builds = 0, g_cache_bytes = 0, g_cache_max_bytes = -1;
uint64_t g_cache_clock = 0;

bool cache_enabled() {
  if (g_cache_enabled < 0) {
    const char* e = std::getenv("AWQ_CDNA4_AUTOCACHE");
    g_cache_enabled = (e && e[0] == '0') ? 0 : 1;
  }
  if (g_cache_max_bytes < 0) {  // AWQ_CDNA4_AUTOCACHE_MAX_GB bounds the second copy of the weights (0 / unset = unbounded)
    const char* e = std::getenv("AWQ_CDNA4_AUTOCACHE_MAX_GB");
    g_cache_max_bytes = e ? (int64_t)(std::atof(e) * (double)(1ull << 30)) : 0;
  }
  if (g_cache_inplace < 0) {
    // AWQ_CDNA4_INPLACE=1: the first call through the reference entry points converts the qweight WHERE IT LIES (via one layer-sized
    // temporary that is freed at once) instead of keeping a permuted second copy: no extra weight memory (35 GB on Llama-3-70B), but
    // the module's `qweight` then holds the cdna4 interleave -- save checkpoints with llm_awq_amd.repacker / cdna4_restore first.
    const char* e = std::getenv("AWQ_CDNA4_INPLACE");
    g_cache_inplace = (e && e[0] == '1') ? 1 : 0;
  }
  return g_cache_enabled == 1;
}

// an in-place entry whose qweight is still alive: put the reference (v2) interleave back before the entry is forgotten, or the next
// call would take the permuted bytes for v2 data and permute them again
void restore_inplace(CacheEntry& e) {
  if (!e.inplace) return;
  at::Tensor t = e.inplace_intact() ? e.inplace_tensor() : at::Tensor();
  e.inplace = false;
  if (!t.defined()) return;  // storage gone, or overwritten with fresh v2 bytes since the conversion: running the cdna4 -> v2 permutation over them would corrupt them
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(t.device());
  hipStream_t st = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (e.built && st != e.build_stream) (void)hipStreamWaitEvent(st, e.built, 0);
  at::Tensor tmp = torch::empty_like(t);
  const int n = (int)t.size(0) * 4, k = (int)t.size(1);
  if (awq_repack_cdna4_to_v2(t.data_ptr(), tmp.data_ptr(), n, k, (void*)st) == AWQ_OK)
    (void)hipMemcpyAsync(t.data_ptr(), tmp.data_ptr(), t.nbytes(), hipMemcpyDeviceToDevice, st);
}

void drop_entry(std::unordered_map<const void*, CacheEntry>::iterator it) {
  if (it->second.c4.defined() && !it->second.inplace) g_cache_bytes -= (int64_t)it->second.c4.nbytes();
  if (it->second.built) (void)hipEventDestroy(it->second.built);
  for (SzSlot& sl : it->second.slot)
    if (sl.built) (void)hipEventDestroy(sl.built);
  g_cache.erase(it);
}

// is this exact buffer (data pointer incl. storage offset) currently held converted in place?  (g_cache_mu held by the caller)
bool inplace_converted_locked(const torch::Tensor& kernel) {
  auto it = g_cache.find(kernel.data_ptr());
  return it != g_cache.end() && it->second.inplace_intact() && it->second.holds(kernel);
}
// the reference-layout kernels must never read a buffer the cache converted where it lies: callers that cannot be served by the cdna4 path
// (cache switched off, fp32 scales, a failed scale pack) get an error that names the way out instead of silently wrong products
void refuse_if_converted(const torch::Tensor& kernel, const char* why) {
  TORCH_CHECK(!inplace_converted_locked(kernel), "awq_inference_engine: this qweight was converted to the cdna4 interleave IN PLACE (AWQ_CDNA4_INPLACE=1) and ",
              why, "; call awq_inference_engine.cdna4_restore(qweight) first");
}

// returns true and fills (c4, szp, szh) when the cdna4 kernels can serve this call (szh stays undefined if the scales are not f16-exact)
bool cdna4_view(const torch::Tensor& kernel, const torch::Tensor& scales, const torch::Tensor& zeros, int64_t n, int64_t k,
                hipStream_t stream, at::Tensor& c4, at::Tensor& szp, at::Tensor* szh = nullptr) {
  if (!cache_enabled() || kernel.scalar_type() != at::kShort ||
      (scales.scalar_type() != at::kBFloat16 && scales.scalar_type() != at::kHalf)) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    refuse_if_converted(kernel, "this call cannot run on the cdna4 kernels (cache disabled, or scales that are neither fp16 nor bf16)");
    return false;
  }
  if (n % 16 != 0 || k % 128 != 0 || kernel.numel() != n / 4 * k) return false;
  // inside a hipGraph capture the weights are never re-packed (an entry built by an earlier warm-up call is used, a first call
  // falls back to the reference-layout kernels); the small scale buffers may be (torch's allocator is capture-safe)
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
  std::lock_guard<std::mutex> lock(g_cache_mu);
  const void* key = kernel.data_ptr();
  auto it = g_cache.find(key);
  if (it != g_cache.end()) {
    auto lw = it->second.w.lock();
    // an in-place entry whose storage was overwritten since the conversion (the shared version counter moved) is stale whichever alias asks
    const bool gone = it->second.inplace && !it->second.inplace_alive();  // its storage was freed and the address handed to another tensor
    const bool overwritten = it->second.inplace && it->second.inplace_alive() && !it->second.inplace_intact();
    if (gone || overwritten || lw.get() != kernel.unsafeGetTensorImpl() || it->second.vw != tensor_version(kernel)) {  // address re-used or edited in place
      CacheEntry& old = it->second;
      const bool same_bytes = old.inplace_intact() && old.holds(kernel);
      if (same_bytes && lw.get() != kernel.unsafeGetTensorImpl()) {
        // ANOTHER tensor over the converted bytes (a view, .detach(), .data, load_state_dict(assign=True) of an alias, a compile wrapper):
        // the storage already holds the cdna4 interleave -- converting "again" would permute it twice.  The entry follows the caller
        // (host-side only: legal inside a capture); a tensor whose version moved under the SAME impl was overwritten with new v2 data.
        old.w = c10::weak_intrusive_ptr<c10::TensorImpl>(kernel.getIntrusivePtr());
        old.vw = tensor_version(kernel);
      } else {
        TORCH_CHECK(!(capturing && (same_bytes || overwritten)), "awq_inference_engine: an in-place converted qweight was modified during a graph capture");
        if (capturing) return false;
        // (same impl, new version: the caller wrote fresh v2 bytes over the buffer -- nothing to restore; a foreign tensor at a re-used
        // address: the old entry's storage is not ours to touch either)
        drop_entry(it);
        it = g_cache.end();
      }
    }
  }
  if (it == g_cache.end()) {
    if (capturing) return false;
    // drop entries whose qweight died or was re-pointed (keeps the map from growing when models are reloaded)
    for (auto i2 = g_cache.begin(); i2 != g_cache.end();) {
      auto cur = i2++;
      auto lw = cur->second.w.lock();
      // (the key is the tensor's data pointer INCLUDING its storage offset: sharded / flattened parameter buffers are views)
      if (cur->second.inplace) {
        // an in-place entry lives exactly as long as the storage it converted: the tensor it last followed may have been a temporary alias, and
        // forgetting the entry while the module's own tensor is alive would have the next call permute the bytes a second time
        if (cur->second.inplace_alive()) continue;
        drop_entry(cur);  // the weights are gone (the cache never held them): nothing to restore
        continue;
      }
      if (!lw || lw->data() != cur->first) drop_entry(cur);
    }
    const int64_t need = (int64_t)kernel.nbytes();
    if (g_cache_inplace != 1 && g_cache_max_bytes > 0 && g_cache_bytes + need > g_cache_max_bytes) return false;  // over budget: reference-layout kernels
    CacheEntry e(kernel);
    if (g_cache_inplace == 1) {
      at::Tensor tmp = torch::empty_like(kernel);  // stream-ordered allocation: returned to the pool when it goes out of scope
      if (awq_repack_v2_to_cdna4(kernel.data_ptr(), tmp.data_ptr(), (int)n, (int)k, (void*)stream) != AWQ_OK) return false;
      if (hipMemcpyAsync(kernel.data_ptr(), tmp.data_ptr(), kernel.nbytes(), hipMemcpyDeviceToDevice, stream) != hipSuccess) return false;
      // (a raw copy: the tensor's version counter does not move, so the entry stays valid)
      e.inplace = true;
      e.ws = c10::weak_intrusive_ptr<c10::StorageImpl>(c10::intrusive_ptr<c10::StorageImpl>::reclaim_copy(kernel.storage().unsafeGetStorageImpl()));
      e.ws_offset = kernel.storage_offset();
      e.ws_n4 = n / 4;
      e.ws_k = k;
      e.ws_dev = kernel.device();
      e.has_vc = !kernel.is_inference();
      if (e.has_vc) e.vc = kernel.unsafeGetTensorImpl()->version_counter();
      e.vc4 = tensor_version(kernel);
    } else {
      e.c4 = torch::empty_like(kernel);
      if (awq_repack_v2_to_cdna4(kernel.data_ptr(), e.c4.data_ptr(), (int)n, (int)k, (void*)stream) != AWQ_OK) return false;
      g_cache_bytes += need;
    }
    if (hipEventCreateWithFlags(&e.built, hipEventDisableTiming) == hipSuccess) (void)hipEventRecord(e.built, stream);
    e.build_stream = stream;
    ++g_cache_builds;
    it = g_cache.emplace(key, std::move(e)).first;
  }
  CacheEntry& e = it->second;
  if (!e.settled && e.built) {
    if (stream != e.build_stream && !capturing) (void)hipStreamWaitEvent(stream, e.built, 0);  // the copy was made on another stream
    if (!capturing && hipEventQuery(e.built) == hipSuccess) e.settled = true;
  }
  // ---- the scale side buffers ----
  SzSlot* hit = nullptr;
  for (SzSlot& sl : e.slot) {
    auto ls = sl.s.lock(), lz = sl.z.lock();
    if (sl.szp.defined() && ls.get() == scales.unsafeGetTensorImpl() && lz.get() == zeros.unsafeGetTensorImpl() &&
        sl.vs == tensor_version(scales) && sl.vz == tensor_version(zeros))
      hit = &sl;
  }
  if (hit == nullptr) {
    // victim: a slot whose (scales, zeros) pair is gone (a prefill call's `scaled_zeros - 8 * scales` temporary) before a live one --
    // two temporaries in a row must not evict the persistent decode pair; among equals the least recently used
    SzSlot* victim = &e.slot[0];
    if (e.slot[0].expired() != e.slot[1].expired()) victim = e.slot[0].expired() ? &e.slot[0] : &e.slot[1];
    else if (e.slot[1].stamp < e.slot[0].stamp) victim = &e.slot[1];
    SzSlot& sl = *victim;
    at::Tensor nszp = torch::empty({n / 16, k / 128, 16}, scales.options().dtype(at::kInt));
    if (awq_pack_sz_cdna4(scales.data_ptr(), zeros.data_ptr(), nszp.data_ptr(), (int)n, (int)k, (void*)stream) != AWQ_OK) {
      refuse_if_converted(kernel, "its scales could not be packed for the cdna4 kernels");
      return false;
    }
    if (capturing) {
      // built while a graph is being captured: the pack kernel is only RECORDED, so the buffer must not be published (an eager call
      // could hit it before the first replay); it lives for this call's launch alone, decode uses the T-typed sz_packed
      c4 = e.inplace ? kernel : e.c4;
      szp = nszp;
      if (szh) *szh = at::Tensor();
      return true;
    }
    at::Tensor nszh;
    if (!capturing) {  // the exactness flag is read back once: not inside a capture (decode then uses sz_packed)
      at::Tensor h = torch::empty({n / 16, k / 128, 16}, scales.options().dtype(at::kInt));
      at::Tensor flag = torch::zeros({1}, scales.options().dtype(at::kInt));
      if (awq_pack_szh_cdna4(scales.data_ptr(), zeros.data_ptr(), h.data_ptr(), (int*)flag.data_ptr(), (int)n, (int)k,
                             scales.scalar_type() == at::kHalf ? AWQ_F16 : AWQ_BF16, (void*)stream) == AWQ_OK &&
          flag.item<int>() == 0)
        nszh = h;
    }
    sl.s = c10::weak_intrusive_ptr<c10::TensorImpl>(scales.getIntrusivePtr());
    sl.z = c10::weak_intrusive_ptr<c10::TensorImpl>(zeros.getIntrusivePtr());
    sl.vs = tensor_version(scales);
    sl.vz = tensor_version(zeros);
    sl.szp = nszp;
    sl.szh = nszh;
    if (!sl.built && hipEventCreateWithFlags(&sl.built, hipEventDisableTiming) != hipSuccess) sl.built = nullptr;
    if (sl.built) (void)hipEventRecord(sl.built, stream);
    sl.build_stream = stream;
    sl.settled = false;
    hit = &sl;
    ++g_cache_sz_builds;
  } else {
    ++g_cache_hits;
    if (!hit->settled && hit->built) {  // packed on another stream: order this one behind it until the event has completed
      if (stream != hit->build_stream && !capturing) (void)hipStreamWaitEvent(stream, hit->built, 0);
      if (!capturing && hipEventQuery(hit->built) == hipSuccess) hit->settled = true;
    }
  }
  hit->stamp = ++g_cache_clock;
  c4 = e.inplace ? kernel : e.c4;  // (in place: the caller's tensor IS the converted buffer)
  szp = hit->szp;
  if (szh) *szh = hit->szh;
  return true;
}

// optional split-K workspace of the cdna4 prefill path (include/awq_cdna4.h); comes from torch's caching allocator, so it is
// stream-ordered and legal inside a graph capture
static at::Tensor cdna4_workspace(const at::Tensor& like, int64_t m, int64_t n, int64_t k, void*& ptr, size_t& bytes) {
  at::Tensor ws;
  ptr = nullptr;
  bytes = awq_w4a16_forward_cdna4_workspace_bytes((int)m, (int)n, (int)k);
  if (bytes) {
    ws = torch::empty({(int64_t)bytes}, like.options().dtype(at::kByte));
    ptr = ws.data_ptr();
  }
  return ws;
}

torch::Tensor gemv_forward_cuda_new(torch::Tensor in_feats, torch::Tensor kernel, torch::Tensor scaling_factors,
                                    torch::Tensor zeros, int m, int n, int k, int group_size) {
  check_inputs(in_feats, kernel, scaling_factors, zeros);
  if (group_size != 128) raise_on(AWQ_ERR_GROUP);
  if (m < 1 || m > 7) raise_on(AWQ_ERR_BATCH);  // the reference's switch(m) covers 1..7 (gemv_cuda.cu:291-329)
  TORCH_CHECK(in_feats.size(-1) == k && in_feats.numel() == (int64_t)m * k, "in_feats must be [m, k]");
  TORCH_CHECK(kernel.numel() == (int64_t)n / 4 * k, "kernel must be int16 [n/4, k]");
  TORCH_CHECK(scaling_factors.size(-1) == n && zeros.size(-1) == n && scaling_factors.size(0) * 128 >= k &&
                  zeros.size(0) * 128 >= k,
              "scales / scaled_zeros must be [Gpad, n]");
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = n;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  at::Tensor c4, szp, szh;
  if (cdna4_view(kernel, scaling_factors, zeros, n, k, stream, c4, szp, &szh)) {
    if (szh.defined())
      raise_on(awq_w4a16_decode_cdna4(in_feats.data_ptr(), c4.data_ptr(), szh.data_ptr(), nullptr, out.data_ptr(), m, n, k, group_size,
                                      dtype_code(in_feats), 0, (void*)stream));
    else
      raise_on(awq_w4a16_forward_cdna4(in_feats.data_ptr(), c4.data_ptr(), scaling_factors.data_ptr(), zeros.data_ptr(), szp.data_ptr(),
                                       nullptr, out.data_ptr(), m, n, k, group_size, dtype_code(in_feats), nullptr, 0, (void*)stream));
    return out;
  }
  raise_on(awq_w4a16_gemv(in_feats.data_ptr(), kernel.data_ptr(), scaling_factors.data_ptr(), zeros.data_ptr(),
                          out.data_ptr(), m, n, k, group_size, dtype_code(in_feats), (void*)stream));
  return out;
}

torch::Tensor gemm_forward_cuda_new(torch::Tensor in_feats, torch::Tensor kernel, torch::Tensor scales,
                                    torch::Tensor zeros) {
  check_inputs(in_feats, kernel, scales, zeros);
  const int64_t n = kernel.size(0) * 4;  // gemm_cuda.cu:1133
  const int64_t k = in_feats.size(-1);   // gemm_cuda.cu:1135
  TORCH_CHECK(k > 0 && in_feats.numel() % k == 0);
  const int64_t m = in_feats.numel() / k;  // gemm_cuda.cu:1134
  TORCH_CHECK(kernel.numel() == n / 4 * k, "kernel must be int16 [n/4, k]");
  TORCH_CHECK(scales.size(-1) == n && zeros.size(-1) == n && scales.size(0) * 128 >= k && zeros.size(0) * 128 >= k,
              "scales / scaled_zeros must be [Gpad, n]");
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = n;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  if (m == 0) return out;
  auto stream = c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  {
    at::Tensor c4, szp, szh;
    if (cdna4_view(kernel, scales, zeros, n, k, stream, c4, szp, &szh)) {
      void* wsp;
      size_t wsb;
      at::Tensor ws = cdna4_workspace(in_feats, m, n, k, wsp, wsb);
      // (round 6: the cached sz_half side buffer -- built for the decode entry when the layer's scales are f16-exact -- serves the prompts too: the tile kernels, the
      // mid-M kernel and the 9 .. 16-row skinny launches dequantise in the f16-mantissa form, as the native modules' calls do; same bits)
      raise_on(awq_w4a16_forward_cdna4_szh(in_feats.data_ptr(), c4.data_ptr(), scales.data_ptr(), zeros.data_ptr(), szp.data_ptr(),
                                           szh.defined() ? szh.data_ptr() : nullptr, nullptr, out.data_ptr(), (int)m, (int)n, (int)k, 128, dtype_code(in_feats), wsp,
                                           wsb, (void*)stream));
      return out;
    }
  }
  const size_t ws_bytes = awq_w4a16_gemm_workspace_bytes((int)m, (int)n, (int)k);
  at::Tensor ws;
  void* wsp = nullptr;
  if (ws_bytes) {
    ws = torch::empty({(int64_t)ws_bytes}, in_feats.options().dtype(at::kByte));
    wsp = ws.data_ptr();
  }
  raise_on(awq_w4a16_gemm(in_feats.data_ptr(), kernel.data_ptr(), scales.data_ptr(), zeros.data_ptr(), out.data_ptr(),
                          (int)m, (int)n, (int)k, 128, dtype_code(in_feats), wsp, ws_bytes, (void*)stream));
  return out;
}

// ---- MI355X-native "cdna4" interleave (bf16): same tensors / shapes, permuted qweight + packed scales ----
torch::Tensor repack_v2_to_cdna4(torch::Tensor kernel) {
  TORCH_CHECK(kernel.is_cuda() && kernel.is_contiguous() && kernel.scalar_type() == at::kShort && kernel.dim() == 2);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(kernel.device());
  at::Tensor out = torch::empty_like(kernel);
  raise_on(awq_repack_v2_to_cdna4(kernel.data_ptr(), out.data_ptr(), (int)kernel.size(0) * 4, (int)kernel.size(1),
                                  (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

torch::Tensor repack_cdna4_to_v2(torch::Tensor kernel) {
  TORCH_CHECK(kernel.is_cuda() && kernel.is_contiguous() && kernel.scalar_type() == at::kShort && kernel.dim() == 2);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(kernel.device());
  at::Tensor out = torch::empty_like(kernel);
  raise_on(awq_repack_cdna4_to_v2(kernel.data_ptr(), out.data_ptr(), (int)kernel.size(0) * 4, (int)kernel.size(1),
                                  (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

torch::Tensor pack_sz_cdna4(torch::Tensor scales, torch::Tensor zeros, int k) {
  TORCH_CHECK(scales.is_cuda() && zeros.is_cuda() && scales.is_contiguous() && zeros.is_contiguous());
  TORCH_CHECK(scales.scalar_type() == zeros.scalar_type() && scales.sizes() == zeros.sizes() && scales.dim() == 2);
  const int64_t n = scales.size(1);
  TORCH_CHECK(n % 16 == 0 && k % 128 == 0 && scales.size(0) * 128 >= k);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(scales.device());
  at::Tensor out = torch::empty({n / 16, k / 128, 16}, scales.options().dtype(at::kInt));
  raise_on(awq_pack_sz_cdna4(scales.data_ptr(), zeros.data_ptr(), out.data_ptr(), (int)n, k,
                             (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// WQLinear.forward on cdna4 buffers: any number of rows (<= 16 -> GEMV kernel), bias optional
torch::Tensor forward_cdna4(torch::Tensor in_feats, torch::Tensor kernel, torch::Tensor scales, torch::Tensor zeros,
                            torch::Tensor sz_packed, c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> sz_half) {
  check_inputs(in_feats, kernel, scales, zeros);
  TORCH_CHECK(in_feats.scalar_type() == at::kBFloat16 || in_feats.scalar_type() == at::kHalf,
              "the cdna4 interleave is defined for bfloat16 / float16");
  TORCH_CHECK(sz_packed.is_cuda() && sz_packed.is_contiguous() && sz_packed.scalar_type() == at::kInt);
  const int64_t n = kernel.size(0) * 4, k = in_feats.size(-1);
  TORCH_CHECK(k > 0 && in_feats.numel() % k == 0 && kernel.numel() == n / 4 * k);
  TORCH_CHECK(sz_packed.numel() == n * (k / 128), "sz_packed must be int32 [n/16, k/128, 16]");
  const int64_t m = in_feats.numel() / k;
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = n;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  if (m == 0) return out;
  const void* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() && bias->scalar_type() == in_feats.scalar_type() && bias->numel() == n);
    bp = bias->data_ptr();
  }
  void* wsp;
  size_t wsb;
  at::Tensor ws = cdna4_workspace(in_feats, m, n, k, wsp, wsb);
  const void* hp = nullptr;  // the layer's sz_half side buffer (pack_szh_cdna4 reported exact): prompts dequantise in the f16-mantissa form
  if (sz_half.has_value() && sz_half->defined()) {
    TORCH_CHECK(sz_half->is_cuda() && sz_half->is_contiguous() && sz_half->scalar_type() == at::kInt && sz_half->numel() == sz_packed.numel());
    hp = sz_half->data_ptr();
  }
  raise_on(awq_w4a16_forward_cdna4_szh(in_feats.data_ptr(), kernel.data_ptr(), scales.data_ptr(), zeros.data_ptr(), sz_packed.data_ptr(), hp, bp,
                                       out.data_ptr(), (int)m, (int)n, (int)k, 128, dtype_code(in_feats), wsp, wsb,
                                       (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// grouped (per-expert) GEMM for MoE layers: tokens sorted by expert, stacked expert weights
torch::Tensor moe_gemm_forward(torch::Tensor x_sorted, torch::Tensor kernel, torch::Tensor scales, torch::Tensor zeros,
                               torch::Tensor expert_offsets, bool cdna4) {
  check_inputs(x_sorted, kernel, scales, zeros);
  TORCH_CHECK(expert_offsets.is_cuda() && expert_offsets.is_contiguous() && expert_offsets.scalar_type() == at::kInt);
  TORCH_CHECK(kernel.dim() == 3 && scales.dim() == 3 && zeros.dim() == 3 && x_sorted.dim() == 2);
  const int64_t e = kernel.size(0), n = kernel.size(1) * 4, k = kernel.size(2), t = x_sorted.size(0);
  TORCH_CHECK(x_sorted.size(1) == k && scales.size(0) == e && scales.size(2) == n && expert_offsets.numel() == e + 1);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x_sorted.device());
  at::Tensor out = torch::empty({t, n}, x_sorted.options());
  raise_on(awq_w4a16_moe_gemm(x_sorted.data_ptr(), kernel.data_ptr(), scales.data_ptr(), zeros.data_ptr(),
                              expert_offsets.data_ptr(), out.data_ptr(), (int)t, (int)e, (int)n, (int)k, (int)scales.size(1), 128,
                              dtype_code(x_sorted), cdna4 ? 1 : 0,
                              (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// grouped forward on cdna4 buffers: decode batches (<= 8 sorted rows) take the grouped GEMV
torch::Tensor moe_forward_cdna4(torch::Tensor x_sorted, torch::Tensor kernel, torch::Tensor scales, torch::Tensor zeros,
                                torch::Tensor sz_packed, torch::Tensor expert_offsets) {
  check_inputs(x_sorted, kernel, scales, zeros);
  TORCH_CHECK(x_sorted.scalar_type() == at::kBFloat16 || x_sorted.scalar_type() == at::kHalf,
              "the cdna4 interleave is defined for bfloat16 / float16");
  TORCH_CHECK(expert_offsets.is_cuda() && expert_offsets.is_contiguous() && expert_offsets.scalar_type() == at::kInt);
  TORCH_CHECK(sz_packed.is_cuda() && sz_packed.is_contiguous() && sz_packed.scalar_type() == at::kInt);
  TORCH_CHECK(kernel.dim() == 3 && scales.dim() == 3 && zeros.dim() == 3 && x_sorted.dim() == 2);
  const int64_t e = kernel.size(0), n = kernel.size(1) * 4, k = kernel.size(2), t = x_sorted.size(0);
  TORCH_CHECK(x_sorted.size(1) == k && scales.size(0) == e && scales.size(2) == n && expert_offsets.numel() == e + 1);
  TORCH_CHECK(sz_packed.numel() == e * n * (k / 128), "sz_packed must be int32 [E, n/16, k/128, 16]");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x_sorted.device());
  at::Tensor out = torch::empty({t, n}, x_sorted.options());
  raise_on(awq_w4a16_moe_forward_cdna4(x_sorted.data_ptr(), kernel.data_ptr(), scales.data_ptr(), zeros.data_ptr(),
                                       sz_packed.data_ptr(), expert_offsets.data_ptr(), out.data_ptr(), (int)t, (int)e, (int)n,
                                       (int)k, (int)scales.size(1), 128, dtype_code(x_sorted),
                                       (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// ---- MoE routing on the device: top-k gate + stable sort by expert, row gather, weighted combine (one launch each) ----
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> moe_route(torch::Tensor router_logits, int64_t top_k,
                                                                                                bool renormalize) {
  TORCH_CHECK(router_logits.is_cuda() && router_logits.is_contiguous() && router_logits.dim() == 2,
              "awq_inference_engine: router_logits must be a contiguous [T, E] GPU tensor");
  const auto st = router_logits.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kBFloat16 || st == at::kHalf, "moe_route: float32 / bfloat16 / float16 logits");
  const int code = st == at::kFloat ? AWQ_F32 : dtype_code(router_logits);
  const int64_t t = router_logits.size(0), e = router_logits.size(1);
  TORCH_CHECK(top_k >= 1 && top_k <= 8 && t >= 1 && t * top_k <= (1 << 20), "moe_route: 1 <= top_k <= 8, 1 <= T, T * top_k <= 2^20");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(router_logits.device());
  const auto iopt = router_logits.options().dtype(at::kInt);
  at::Tensor ids = torch::empty({t, top_k}, iopt), w = torch::empty({t, top_k}, router_logits.options().dtype(at::kFloat));
  at::Tensor order = torch::empty({t * top_k}, iopt), inv = torch::empty({t * top_k}, iopt), offsets = torch::empty({e + 1}, iopt);
  raise_on(awq_moe_route(router_logits.data_ptr(), code, (int)t, (int)e, (int)top_k, renormalize ? 1 : 0, ids.data_ptr(), w.data_ptr(), order.data_ptr(),
                         inv.data_ptr(), offsets.data_ptr(), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return {ids, w, order, inv, offsets};
}

torch::Tensor moe_gather(torch::Tensor x, torch::Tensor order, int64_t top_k) {
  TORCH_CHECK(x.is_cuda() && x.is_contiguous() && x.dim() == 2 && order.is_cuda() && order.is_contiguous() && order.scalar_type() == at::kInt,
              "awq_inference_engine: x must be a contiguous [T, H] GPU tensor and order int32 on the GPU");
  TORCH_CHECK(top_k >= 1 && order.numel() == x.size(0) * top_k, "moe_gather: order must hold T * top_k slots");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  at::Tensor xs = torch::empty({order.numel(), x.size(1)}, x.options());
  raise_on(awq_moe_gather(x.data_ptr(), order.data_ptr(), xs.data_ptr(), (int)x.size(0), (int)top_k, (int)x.size(1), dtype_code(x),
                          (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return xs;
}

torch::Tensor moe_combine(torch::Tensor ys, torch::Tensor inv, torch::Tensor topk_w) {
  TORCH_CHECK(ys.is_cuda() && ys.is_contiguous() && ys.dim() == 2 && inv.is_cuda() && inv.is_contiguous() && inv.scalar_type() == at::kInt &&
                  topk_w.is_cuda() && topk_w.is_contiguous() && topk_w.dim() == 2 && topk_w.scalar_type() == at::kFloat,
              "awq_inference_engine: ys [T * k, H], inv int32 [T * k] and topk_w float32 [T, k] must be contiguous GPU tensors");
  const int64_t t = topk_w.size(0), k = topk_w.size(1);
  TORCH_CHECK(inv.numel() == t * k && ys.size(0) == t * k, "moe_combine: ys / inv must hold T * k rows");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(ys.device());
  at::Tensor out = torch::empty({t, ys.size(1)}, ys.options());
  raise_on(awq_moe_combine(ys.data_ptr(), inv.data_ptr(), topk_w.data_ptr(), out.data_ptr(), (int)t, (int)k, (int)ys.size(1), dtype_code(ys),
                           (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// ---- next-token sampling on the device: logits [B, V] -> tokens int32 [B], one launch, every parameter an optional per-row GPU tensor ----
torch::Tensor sample_logits(torch::Tensor logits, torch::Tensor u, c10::optional<torch::Tensor> temperature, c10::optional<torch::Tensor> top_k,
                            c10::optional<torch::Tensor> top_p, c10::optional<torch::Tensor> repetition_penalty,
                            c10::optional<torch::Tensor> history, c10::optional<torch::Tensor> hist_len, c10::optional<torch::Tensor> seqlens,
                            c10::optional<torch::Tensor> stop_ids, c10::optional<torch::Tensor> finished, int64_t max_len, bool append, bool advance) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, "awq_inference_engine: logits must be a contiguous [B, V] GPU tensor");
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kBFloat16 || st == at::kHalf, "sample_logits: float32 / bfloat16 / float16 logits");
  const int code = st == at::kFloat ? AWQ_F32 : dtype_code(logits);
  const int64_t b = logits.size(0), v = logits.size(1);
  auto row = [&](const c10::optional<torch::Tensor>& t, at::ScalarType want, const char* name) -> void* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == want && t->numel() == b && t->device() == logits.device(),
                "sample_logits: ", name, " must be a contiguous [B] GPU tensor of its dtype");
    return t->data_ptr();
  };
  TORCH_CHECK(u.is_cuda() && u.is_contiguous() && u.scalar_type() == at::kFloat && u.numel() == b, "sample_logits: u must be float32 [B] on the GPU");
  TORCH_CHECK(history.has_value() == hist_len.has_value(), "sample_logits: history and hist_len come together");
  void* hist = nullptr;
  int64_t lh = 0;
  if (history.has_value()) {
    TORCH_CHECK(history->is_cuda() && history->is_contiguous() && history->scalar_type() == at::kInt && history->dim() == 2 &&
                    history->size(0) == b && history->size(1) >= 1,
                "sample_logits: history must be a contiguous int32 [B, Lh] GPU tensor");
    hist = history->data_ptr();
    lh = history->size(1);
  }
  void* stops = nullptr;
  int64_t ns = 0;
  if (stop_ids.has_value()) {
    TORCH_CHECK(stop_ids->is_cuda() && stop_ids->is_contiguous() && stop_ids->scalar_type() == at::kInt && stop_ids->dim() == 1,
                "sample_logits: stop_ids must be a contiguous int32 [S] GPU tensor");
    stops = stop_ids->data_ptr();
    ns = stop_ids->numel();
  }
  TORCH_CHECK(!append || hist, "sample_logits: append needs history and hist_len");
  TORCH_CHECK(!advance || seqlens.has_value(), "sample_logits: advance needs seqlens");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  at::Tensor tokens = torch::empty({b}, logits.options().dtype(at::kInt));
  raise_on(awq_sample_logits(logits.data_ptr(), code, (int)b, (int)v, u.data_ptr(), row(temperature, at::kFloat, "temperature"),
                             row(top_k, at::kInt, "top_k"), row(top_p, at::kFloat, "top_p"), row(repetition_penalty, at::kFloat, "repetition_penalty"),
                             hist, row(hist_len, at::kInt, "hist_len"), (int)lh, row(seqlens, at::kInt, "seqlens"), stops, (int)ns,
                             row(finished, at::kInt, "finished"), (int)max_len, (append ? AWQ_SAMPLE_APPEND : 0) | (advance ? AWQ_SAMPLE_ADVANCE : 0),
                             tokens.data_ptr(), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return tokens;
}

// ---- prompt-lookup speculative decoding on the device: drafter, packer, packed verifier and accept chain (awq_spec_*) ----
namespace {
// a contiguous int32 GPU tensor of n elements (n < 0: any size) on `dev` -> its pointer; nullptr for an absent optional
void* spec_i32(const torch::Tensor& t, int64_t n, const at::Device& dev, const char* who, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kInt && t.device() == dev && (n < 0 || t.numel() == n), who, ": ", name,
              " must be a contiguous int32 GPU tensor of its documented size");
  return t.data_ptr();
}
void* spec_i32(const c10::optional<torch::Tensor>& t, int64_t n, const at::Device& dev, const char* who, const char* name) {
  return t.has_value() ? spec_i32(*t, n, dev, who, name) : nullptr;
}
void* spec_f32(const c10::optional<torch::Tensor>& t, int64_t n, const at::Device& dev, const char* who, const char* name) {
  if (!t.has_value()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == at::kFloat && t->device() == dev && t->numel() == n, who, ": ", name,
              " must be a contiguous float32 [B] GPU tensor");
  return t->data_ptr();
}
}  // namespace

std::vector<torch::Tensor> spec_draft_ngram(torch::Tensor history, torch::Tensor hist_len, torch::Tensor seqlens, int64_t vocab, int64_t kmax,
                                            int64_t ngram_min, int64_t ngram_max, int64_t max_len, c10::optional<torch::Tensor> max_draft) {
  const char* who = "spec_draft_ngram";
  TORCH_CHECK(history.dim() == 2 && history.size(1) >= 1, who, ": history must be int32 [B, Lh]");
  const auto dev = history.device();
  const int64_t b = history.size(0);
  spec_i32(history, -1, dev, who, "history");
  TORCH_CHECK(kmax >= 0 && kmax <= 15, who, ": 0 <= kmax <= 15");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
  at::Tensor drafts = torch::empty({b, kmax}, history.options()), draft_len = torch::empty({b}, history.options());
  raise_on(awq_spec_draft_ngram(history.data_ptr(), spec_i32(hist_len, b, dev, who, "hist_len"), spec_i32(seqlens, b, dev, who, "seqlens"),
                                spec_i32(max_draft, b, dev, who, "max_draft"), kmax > 0 ? drafts.data_ptr() : nullptr, draft_len.data_ptr(), (int)b,
                                (int)history.size(1), (int)vocab, (int)kmax, (int)ngram_min, (int)ngram_max, (int)max_len,
                                (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return {drafts, draft_len};
}

std::vector<torch::Tensor> spec_pack(torch::Tensor last_tokens, torch::Tensor drafts, torch::Tensor draft_len, torch::Tensor seqlens, int64_t total_q) {
  const char* who = "spec_pack";
  const auto dev = last_tokens.device();
  const int64_t b = last_tokens.numel();
  TORCH_CHECK(drafts.dim() == 2 && drafts.size(0) == b, who, ": drafts must be int32 [B, kmax]");
  TORCH_CHECK(total_q >= b && b >= 1, who, ": total_q >= B >= 1");
  const int64_t kmax = drafts.size(1);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
  at::Tensor cu = torch::empty({b + 1}, last_tokens.options()), ids = torch::empty({total_q}, last_tokens.options());
  raise_on(awq_spec_pack(spec_i32(last_tokens, b, dev, who, "last_tokens"), kmax > 0 ? spec_i32(drafts, -1, dev, who, "drafts") : nullptr,
                         spec_i32(draft_len, b, dev, who, "draft_len"), spec_i32(seqlens, b, dev, who, "seqlens"), cu.data_ptr(), ids.data_ptr(),
                         (int)b, (int)kmax, (int)total_q, (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return {cu, ids};
}

torch::Tensor spec_verify(torch::Tensor logits, torch::Tensor u, torch::Tensor cu_seqlens_q, torch::Tensor input_ids,
                          c10::optional<torch::Tensor> temperature, c10::optional<torch::Tensor> top_k, c10::optional<torch::Tensor> top_p,
                          c10::optional<torch::Tensor> repetition_penalty, c10::optional<torch::Tensor> history, c10::optional<torch::Tensor> hist_len) {
  const char* who = "spec_verify";
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2, "awq_inference_engine: logits must be a contiguous [total_q, V] GPU tensor");
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kBFloat16 || st == at::kHalf, who, ": float32 / bfloat16 / float16 logits");
  const int code = st == at::kFloat ? AWQ_F32 : dtype_code(logits);
  const auto dev = logits.device();
  const int64_t tq = logits.size(0), v = logits.size(1), b = cu_seqlens_q.numel() - 1;
  TORCH_CHECK(b >= 1, who, ": cu_seqlens_q must be int32 [B + 1]");
  TORCH_CHECK(u.is_cuda() && u.is_contiguous() && u.scalar_type() == at::kFloat && u.numel() == tq, who, ": u must be float32 [total_q] on the GPU");
  TORCH_CHECK(history.has_value() == hist_len.has_value(), who, ": history and hist_len come together");
  int64_t lh = 0;
  if (history.has_value()) {
    TORCH_CHECK(history->dim() == 2 && history->size(0) == b && history->size(1) >= 1, who, ": history must be int32 [B, Lh]");
    lh = history->size(1);
  }
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
  at::Tensor row_tokens = torch::empty({tq}, logits.options().dtype(at::kInt));
  raise_on(awq_spec_verify(logits.data_ptr(), code, (int)tq, (int)v, u.data_ptr(), spec_i32(cu_seqlens_q, b + 1, dev, who, "cu_seqlens_q"),
                           spec_i32(input_ids, tq, dev, who, "input_ids"), (int)b, spec_f32(temperature, b, dev, who, "temperature"),
                           spec_i32(top_k, b, dev, who, "top_k"), spec_f32(top_p, b, dev, who, "top_p"),
                           spec_f32(repetition_penalty, b, dev, who, "repetition_penalty"), spec_i32(history, -1, dev, who, "history"),
                           spec_i32(hist_len, b, dev, who, "hist_len"), (int)lh, row_tokens.data_ptr(),
                           (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return row_tokens;
}

std::vector<torch::Tensor> spec_accept(torch::Tensor row_tokens, torch::Tensor input_ids, torch::Tensor cu_seqlens_q, int64_t kmax,
                                       c10::optional<torch::Tensor> history, c10::optional<torch::Tensor> hist_len,
                                       c10::optional<torch::Tensor> seqlens, c10::optional<torch::Tensor> stop_ids,
                                       c10::optional<torch::Tensor> finished, int64_t max_len, bool append, bool advance) {
  const char* who = "spec_accept";
  const auto dev = row_tokens.device();
  const int64_t tq = row_tokens.numel(), b = cu_seqlens_q.numel() - 1;
  TORCH_CHECK(b >= 1 && tq >= 1, who, ": cu_seqlens_q must be int32 [B + 1] and row_tokens [total_q]");
  TORCH_CHECK(kmax >= 0 && kmax <= 15, who, ": 0 <= kmax <= 15");
  TORCH_CHECK(history.has_value() == hist_len.has_value(), who, ": history and hist_len come together");
  int64_t lh = 0;
  if (history.has_value()) {
    TORCH_CHECK(history->dim() == 2 && history->size(0) == b && history->size(1) >= 1, who, ": history must be int32 [B, Lh]");
    lh = history->size(1);
  }
  TORCH_CHECK(!append || history.has_value(), who, ": append needs history and hist_len");
  TORCH_CHECK(!advance || seqlens.has_value(), who, ": advance needs seqlens");
  TORCH_CHECK(!stop_ids.has_value() || stop_ids->dim() == 1, who, ": stop_ids must be int32 [S]");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(dev);
  const auto opt = row_tokens.options();
  at::Tensor out = torch::empty({b, kmax + 1}, opt), num = torch::empty({b}, opt), last = torch::empty({b}, opt);
  raise_on(awq_spec_accept(spec_i32(row_tokens, tq, dev, who, "row_tokens"), spec_i32(input_ids, tq, dev, who, "input_ids"),
                           spec_i32(cu_seqlens_q, b + 1, dev, who, "cu_seqlens_q"), (int)b, (int)tq, (int)kmax,
                           spec_i32(history, -1, dev, who, "history"), spec_i32(hist_len, b, dev, who, "hist_len"), (int)lh,
                           spec_i32(seqlens, b, dev, who, "seqlens"), spec_i32(stop_ids, -1, dev, who, "stop_ids"),
                           stop_ids.has_value() ? (int)stop_ids->numel() : 0, spec_i32(finished, b, dev, who, "finished"), (int)max_len,
                           (append ? AWQ_SAMPLE_APPEND : 0) | (advance ? AWQ_SAMPLE_ADVANCE : 0), out.data_ptr(), num.data_ptr(), last.data_ptr(),
                           (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return {out, num, last};
}

// ---- LM head for decode (final RMSNorm + vocabulary GEMV, one launch) and the token embedding gather that takes the sampler's -1 ----
// a cap as the C ABI takes it: finite and not negative, 0 = no cap
static float checked_softcap(const char* who, double softcap) {
  const float cap = (float)softcap;
  TORCH_CHECK(softcap >= 0.0 && cap <= 3.4028234663852886e38f, who, ": softcap ", softcap, " must be finite and not negative (0: no cap)");
  return cap;
}

static torch::Tensor lm_head_impl(torch::Tensor x, torch::Tensor weight, c10::optional<torch::Tensor> gamma, double eps,
                                  c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> seqlens, c10::optional<torch::Tensor> out,
                                  at::ScalarType out_dtype, int64_t max_blocks, float softcap) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && (x.stride(1) == 1 || x.size(1) <= 1), "awq_inference_engine: lm_head: x must be a [M, K] GPU tensor with a contiguous last dimension");
  TORCH_CHECK(weight.is_cuda() && weight.is_contiguous() && weight.dim() == 2 && weight.size(1) == x.size(1) && weight.scalar_type() == x.scalar_type(),
              "lm_head: weight must be a contiguous [V, K] GPU tensor of x's dtype");
  const int code = dtype_code(x);
  const int64_t m = x.size(0), k = x.size(1), v = weight.size(0);
  auto vec = [&](const c10::optional<torch::Tensor>& t, at::ScalarType want, int64_t n, const char* name) -> void* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == want && t->numel() == n && t->device() == x.device(), "lm_head: ", name,
                " must be a contiguous GPU tensor of its size and dtype");
    return t->data_ptr();
  };
  TORCH_CHECK(out_dtype == at::kFloat || out_dtype == x.scalar_type(), "lm_head: out_dtype must be float32 or x's dtype");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  at::Tensor o;
  if (out.has_value()) {
    o = *out;
    TORCH_CHECK(o.is_cuda() && o.is_contiguous() && o.dim() == 2 && o.size(0) == m && o.size(1) == v && o.scalar_type() == out_dtype &&
                    o.device() == x.device(),
                "lm_head: out must be a contiguous [M, V] tensor of out_dtype on x's device");
  } else {
    o = seqlens.has_value() ? torch::zeros({m, v}, x.options().dtype(out_dtype)) : torch::empty({m, v}, x.options().dtype(out_dtype));
  }
  const int64_t ldx = m > 1 ? x.stride(0) : std::max<int64_t>(x.stride(0), k) / 8 * 8;
  raise_on(awq_lm_head_softcap(x.data_ptr(), (long)ldx, vec(gamma, x.scalar_type(), k, "gamma"), (float)eps, weight.data_ptr(),
                               vec(bias, x.scalar_type(), v, "bias"), (const int*)vec(seqlens, at::kInt, m, "seqlens"), o.data_ptr(),
                               out_dtype == at::kFloat ? AWQ_F32 : code, (int)m, (int)v, (int)k, code, softcap, (int)max_blocks,
                               (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return o;
}

torch::Tensor lm_head(torch::Tensor x, torch::Tensor weight, c10::optional<torch::Tensor> gamma, double eps, c10::optional<torch::Tensor> bias,
                      c10::optional<torch::Tensor> seqlens, c10::optional<torch::Tensor> out, at::ScalarType out_dtype, int64_t max_blocks) {
  return lm_head_impl(x, weight, gamma, eps, bias, seqlens, out, out_dtype, max_blocks, 0.f);  // softcap 0: awq_lm_head itself
}

// lm_head with every logit capped in the epilogue: softcap * tanh(y / softcap) on the fp32 sum behind the bias, before the one rounding
torch::Tensor lm_head_softcap(torch::Tensor x, torch::Tensor weight, double softcap, c10::optional<torch::Tensor> gamma, double eps,
                              c10::optional<torch::Tensor> bias, c10::optional<torch::Tensor> seqlens, c10::optional<torch::Tensor> out,
                              at::ScalarType out_dtype, int64_t max_blocks) {
  return lm_head_impl(x, weight, gamma, eps, bias, seqlens, out, out_dtype, max_blocks, checked_softcap("lm_head_softcap", softcap));
}

// logits [B, V] that already exist, capped in place; rows with seqlens < 0 untouched.  Returns logits
torch::Tensor logit_softcap_(torch::Tensor logits, double softcap, c10::optional<torch::Tensor> seqlens) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && (logits.stride(1) == 1 || logits.size(1) <= 1),
              "awq_inference_engine: logit_softcap_: logits must be a [B, V] GPU tensor with a contiguous last dimension");
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16, "logit_softcap_: logits must be float32, bfloat16 or float16");
  const int64_t b = logits.size(0), v = logits.size(1);
  TORCH_CHECK(!seqlens.has_value() || (seqlens->is_cuda() && seqlens->is_contiguous() && seqlens->scalar_type() == at::kInt && seqlens->numel() == b &&
                                       seqlens->device() == logits.device()),
              "logit_softcap_: seqlens must be a contiguous int32 [B] tensor on the logits' device");
  const float cap = checked_softcap("logit_softcap_", softcap);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  const int64_t ld = b > 1 ? logits.stride(0) : std::max<int64_t>(logits.stride(0), v);
  raise_on(awq_logit_softcap(logits.data_ptr(), st == at::kFloat ? AWQ_F32 : (st == at::kHalf ? AWQ_F16 : AWQ_BF16), (long)ld,
                             seqlens.has_value() ? (const int*)seqlens->data_ptr() : nullptr, (int)b, (int)v, cap,
                             (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return logits;
}

torch::Tensor embed_tokens(torch::Tensor tokens, torch::Tensor table) {
  TORCH_CHECK(tokens.is_cuda() && tokens.is_contiguous() && tokens.scalar_type() == at::kInt, "awq_inference_engine: embed_tokens: tokens must be a contiguous int32 GPU tensor");
  TORCH_CHECK(table.is_cuda() && table.is_contiguous() && table.dim() == 2 && table.device() == tokens.device(),
              "embed_tokens: table must be a contiguous [V, K] GPU tensor on the tokens' device");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(table.device());
  auto shape = tokens.sizes().vec();
  shape.push_back(table.size(1));
  at::Tensor out = torch::empty(shape, table.options());
  if (tokens.numel() == 0) return out;
  raise_on(awq_embed_tokens((const int*)tokens.data_ptr(), table.data_ptr(), out.data_ptr(), (int)tokens.numel(), (int)table.size(0), (int)table.size(1),
                            dtype_code(table), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// ---- Token log-probabilities: LM head fused with log-sum-exp; returns (logprob, lse, target_logit, argmax), zero-filled where a row is ignored (and
//      logprob / target_logit all zeros without targets) ----
static std::vector<torch::Tensor> lm_head_logprobs_impl(torch::Tensor x, torch::Tensor weight, c10::optional<torch::Tensor> targets,
                                                       c10::optional<torch::Tensor> gamma, double eps, c10::optional<torch::Tensor> bias,
                                                       bool round_logits, int64_t max_blocks, float softcap) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && (x.stride(1) == 1 || x.size(1) <= 1),
              "awq_inference_engine: lm_head_logprobs: x must be a [T, K] GPU tensor with a contiguous last dimension");
  TORCH_CHECK(weight.is_cuda() && weight.is_contiguous() && weight.dim() == 2 && weight.size(1) == x.size(1) && weight.scalar_type() == x.scalar_type(),
              "lm_head_logprobs: weight must be a contiguous [V, K] GPU tensor of x's dtype");
  if (gamma.has_value()) x = x.contiguous();
  const int code = dtype_code(x);
  const int64_t t = x.size(0), k = x.size(1), v = weight.size(0);
  auto vec = [&](const c10::optional<torch::Tensor>& a, at::ScalarType want, int64_t n, const char* name) -> void* {
    if (!a.has_value()) return nullptr;
    TORCH_CHECK(a->is_cuda() && a->is_contiguous() && a->scalar_type() == want && a->numel() == n && a->device() == x.device(), "lm_head_logprobs: ",
                name, " must be a contiguous GPU tensor of its size and dtype");
    return a->data_ptr();
  };
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const auto f32 = x.options().dtype(at::kFloat);
  at::Tensor logprob = torch::zeros({t}, f32), lse = torch::zeros({t}, f32), tl = torch::zeros({t}, f32),
             argmax = torch::zeros({t}, x.options().dtype(at::kInt));
  const size_t bytes = awq_lm_head_logprobs_workspace_bytes((int)t, (int)v, (int)k, gamma.has_value() ? 1 : 0);
  at::Tensor ws = torch::empty({(int64_t)bytes}, x.options().dtype(at::kByte));
  const int64_t ldx = gamma.has_value() ? k : (t > 1 ? x.stride(0) : std::max<int64_t>(x.stride(0), k) / 8 * 8);
  const bool tg = targets.has_value();
  raise_on(awq_lm_head_logprobs_softcap(x.data_ptr(), (long)ldx, vec(gamma, x.scalar_type(), k, "gamma"), (float)eps, weight.data_ptr(),
                                        vec(bias, x.scalar_type(), v, "bias"), (const int*)vec(targets, at::kInt, t, "targets"),
                                        tg ? (float*)logprob.data_ptr() : nullptr, (float*)lse.data_ptr(), tg ? (float*)tl.data_ptr() : nullptr,
                                        (int*)argmax.data_ptr(), (int)t, (int)v, (int)k, code, round_logits ? 1 : 0, softcap, ws.data_ptr(), bytes,
                                        (int)max_blocks, (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return {logprob, lse, tl, argmax};
}

std::vector<torch::Tensor> lm_head_logprobs(torch::Tensor x, torch::Tensor weight, c10::optional<torch::Tensor> targets,
                                            c10::optional<torch::Tensor> gamma, double eps, c10::optional<torch::Tensor> bias, bool round_logits,
                                            int64_t max_blocks) {
  return lm_head_logprobs_impl(x, weight, targets, gamma, eps, bias, round_logits, max_blocks, 0.f);  // softcap 0: awq_lm_head_logprobs itself
}

// lm_head_logprobs with every logit capped before the max / sum-exp, the target pick and the argmax
std::vector<torch::Tensor> lm_head_logprobs_softcap(torch::Tensor x, torch::Tensor weight, double softcap, c10::optional<torch::Tensor> targets,
                                                    c10::optional<torch::Tensor> gamma, double eps, c10::optional<torch::Tensor> bias,
                                                    bool round_logits, int64_t max_blocks) {
  return lm_head_logprobs_impl(x, weight, targets, gamma, eps, bias, round_logits, max_blocks, checked_softcap("lm_head_logprobs_softcap", softcap));
}

// (logprob, lse, argmax) of logits [B, V] that already exist
std::vector<torch::Tensor> token_logprobs(torch::Tensor logits, c10::optional<torch::Tensor> targets) {
  TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && (logits.stride(1) == 1 || logits.size(1) <= 1),
              "awq_inference_engine: token_logprobs: logits must be a [B, V] GPU tensor with a contiguous last dimension");
  const auto st = logits.scalar_type();
  TORCH_CHECK(st == at::kFloat || st == at::kHalf || st == at::kBFloat16, "token_logprobs: logits must be float32, bfloat16 or float16");
  const int64_t b = logits.size(0), v = logits.size(1);
  TORCH_CHECK(!targets.has_value() || (targets->is_cuda() && targets->is_contiguous() && targets->scalar_type() == at::kInt && targets->numel() == b &&
                                       targets->device() == logits.device()),
              "token_logprobs: targets must be a contiguous int32 [B] tensor on the logits' device");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(logits.device());
  const auto f32 = logits.options().dtype(at::kFloat);
  at::Tensor logprob = torch::zeros({b}, f32), lse = torch::zeros({b}, f32), argmax = torch::zeros({b}, logits.options().dtype(at::kInt));
  const int64_t ld = b > 1 ? logits.stride(0) : std::max<int64_t>(logits.stride(0), v);
  raise_on(awq_token_logprobs(logits.data_ptr(), st == at::kFloat ? AWQ_F32 : (st == at::kHalf ? AWQ_F16 : AWQ_BF16), (long)ld,
                              targets.has_value() ? (const int*)targets->data_ptr() : nullptr,
                              targets.has_value() ? (float*)logprob.data_ptr() : nullptr, (float*)lse.data_ptr(), (int*)argmax.data_ptr(), (int)b,
                              (int)v, (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return {logprob, lse, argmax};
}

// ---- Multi-LoRA on packed steps: shrink (x A_a^T into the fp32 K-split workspace) and expand (scale, round, B_a^T, add into y in place) ----
struct LoraBatch {
  const int* ids;
  const int* cu;
  int batch, max_seqlen_q, total_q;
};

LoraBatch lora_batch(const char* who, const torch::Tensor& rows, const torch::Tensor& adapter_ids, const c10::optional<torch::Tensor>& cu_seqlens_q,
                     int64_t max_seqlen_q) {
  TORCH_CHECK(adapter_ids.is_cuda() && adapter_ids.is_contiguous() && adapter_ids.scalar_type() == at::kInt && adapter_ids.dim() == 1 &&
                  adapter_ids.numel() >= 1 && adapter_ids.device() == rows.device(),
              "awq_inference_engine: ", who, ": adapter_ids must be a contiguous int32 [B] tensor on the rows' GPU");
  const int64_t b = adapter_ids.numel();
  if (cu_seqlens_q.has_value())
    TORCH_CHECK(cu_seqlens_q->is_cuda() && cu_seqlens_q->is_contiguous() && cu_seqlens_q->scalar_type() == at::kInt && cu_seqlens_q->dim() == 1 &&
                    cu_seqlens_q->numel() == b + 1 && cu_seqlens_q->device() == rows.device(),
                "awq_inference_engine: ", who, ": cu_seqlens_q must be a contiguous int32 [B + 1] tensor on the rows' GPU");
  return {(const int*)adapter_ids.data_ptr(), cu_seqlens_q.has_value() ? (const int*)cu_seqlens_q->data_ptr() : nullptr, (int)b, (int)max_seqlen_q,
          (int)rows.size(0)};
}

void lora_ws_check(const char* who, const torch::Tensor& ws, const torch::Tensor& rows) {
  TORCH_CHECK(ws.is_cuda() && ws.is_contiguous() && ws.scalar_type() == at::kFloat && ws.device() == rows.device(), "awq_inference_engine: ", who,
              ": ws must be a contiguous float32 tensor on the rows' GPU");
}

torch::Tensor lora_shrink(torch::Tensor x, torch::Tensor a_pool, torch::Tensor adapter_ids, torch::Tensor ws, int64_t rank,
                          c10::optional<torch::Tensor> cu_seqlens_q, int64_t max_seqlen_q) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.size(0) >= 1 && (x.stride(1) == 1 || x.size(1) <= 1),
              "awq_inference_engine: lora_shrink: x must be a [total_q, K] GPU tensor with a contiguous last dimension");
  TORCH_CHECK(a_pool.is_cuda() && a_pool.is_contiguous() && a_pool.dim() == 3 && a_pool.size(2) == x.size(1) && a_pool.scalar_type() == x.scalar_type() &&
                  a_pool.device() == x.device() && rank >= 1 && a_pool.size(1) % rank == 0,
              "awq_inference_engine: lora_shrink: a_pool must be a contiguous [S, n_slices * R, K] GPU tensor of x's dtype");
  lora_ws_check("lora_shrink", ws, x);
  const LoraBatch lb = lora_batch("lora_shrink", x, adapter_ids, cu_seqlens_q, max_seqlen_q);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  const int64_t ldx = x.size(0) > 1 ? x.stride(0) : std::max<int64_t>(x.stride(0), x.size(1)) / 8 * 8;
  raise_on(awq_lora_shrink(x.data_ptr(), (long)ldx, a_pool.data_ptr(), lb.ids, lb.cu, ws.data_ptr(), (size_t)ws.numel() * 4, lb.batch, lb.max_seqlen_q,
                           lb.total_q, (int)a_pool.size(0), (int)x.size(1), (int)rank, (int)(a_pool.size(1) / rank), dtype_code(x),
                           (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return ws;
}

torch::Tensor lora_expand(torch::Tensor ws, torch::Tensor b_pool, torch::Tensor scaling, torch::Tensor adapter_ids, torch::Tensor y, int64_t k,
                          std::vector<int64_t> slice_end, c10::optional<torch::Tensor> cu_seqlens_q, int64_t max_seqlen_q) {
  TORCH_CHECK(y.is_cuda() && y.is_contiguous() && y.dim() == 2 && y.size(0) >= 1, "awq_inference_engine: lora_expand: y must be a contiguous [total_q, N] GPU tensor");
  TORCH_CHECK(b_pool.is_cuda() && b_pool.is_contiguous() && b_pool.dim() == 3 && b_pool.size(1) == y.size(1) && b_pool.scalar_type() == y.scalar_type() &&
                  b_pool.device() == y.device(),
              "awq_inference_engine: lora_expand: b_pool must be a contiguous [S, N, R] GPU tensor of y's dtype");
  TORCH_CHECK(scaling.is_cuda() && scaling.is_contiguous() && scaling.scalar_type() == at::kFloat && scaling.numel() == b_pool.size(0) &&
                  scaling.device() == y.device(),
              "awq_inference_engine: lora_expand: scaling must be a contiguous float32 [S] tensor on y's GPU");
  TORCH_CHECK(slice_end.size() >= 1 && slice_end.size() <= 3, "awq_inference_engine: lora_expand: slice_end must hold 1 .. 3 column ends");
  lora_ws_check("lora_expand", ws, y);
  const LoraBatch lb = lora_batch("lora_expand", y, adapter_ids, cu_seqlens_q, max_seqlen_q);
  int ends[3] = {0, 0, 0};
  for (size_t j = 0; j < slice_end.size(); ++j) ends[j] = (int)slice_end[j];
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y.device());
  raise_on(awq_lora_expand(ws.data_ptr(), (size_t)ws.numel() * 4, b_pool.data_ptr(), (const float*)scaling.data_ptr(), lb.ids, lb.cu, y.data_ptr(),
                           lb.batch, lb.max_seqlen_q, lb.total_q, (int)b_pool.size(0), (int)y.size(1), (int)k, (int)b_pool.size(2), ends,
                           (int)slice_end.size(), dtype_code(y), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return y;
}

// expand on QuantLlamaMLP's gate / up pair: h [total_q, F] = silu(gate') * up' from the unfused interleaved output y2 [total_q, 2F] (read only)
torch::Tensor lora_expand_gate_up(torch::Tensor ws, torch::Tensor b_pool, torch::Tensor scaling, torch::Tensor adapter_ids, torch::Tensor y2, int64_t k,
                                  c10::optional<torch::Tensor> h, c10::optional<torch::Tensor> cu_seqlens_q, int64_t max_seqlen_q) {
  TORCH_CHECK(y2.is_cuda() && y2.is_contiguous() && y2.dim() == 2 && y2.size(0) >= 1 && y2.size(1) >= 16 && y2.size(1) % 16 == 0,
              "awq_inference_engine: lora_expand_gate_up: y2 must be a contiguous [total_q, 2F] GPU tensor, 2F a multiple of 16");
  TORCH_CHECK(b_pool.is_cuda() && b_pool.is_contiguous() && b_pool.dim() == 3 && b_pool.size(1) == y2.size(1) && b_pool.scalar_type() == y2.scalar_type() &&
                  b_pool.device() == y2.device(),
              "awq_inference_engine: lora_expand_gate_up: b_pool must be a contiguous [S, 2F, R] GPU tensor of y2's dtype");
  TORCH_CHECK(scaling.is_cuda() && scaling.is_contiguous() && scaling.scalar_type() == at::kFloat && scaling.numel() == b_pool.size(0) &&
                  scaling.device() == y2.device(),
              "awq_inference_engine: lora_expand_gate_up: scaling must be a contiguous float32 [S] tensor on y2's GPU");
  lora_ws_check("lora_expand_gate_up", ws, y2);
  const LoraBatch lb = lora_batch("lora_expand_gate_up", y2, adapter_ids, cu_seqlens_q, max_seqlen_q);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(y2.device());
  torch::Tensor out = h.has_value() ? *h : torch::empty({y2.size(0), y2.size(1) / 2}, y2.options());
  TORCH_CHECK(out.is_cuda() && out.is_contiguous() && out.dim() == 2 && out.size(0) == y2.size(0) && out.size(1) * 2 == y2.size(1) &&
                  out.scalar_type() == y2.scalar_type() && out.device() == y2.device(),
              "awq_inference_engine: lora_expand_gate_up: h must be a contiguous [total_q, F] GPU tensor of y2's dtype");
  raise_on(awq_lora_expand_gate_up(ws.data_ptr(), (size_t)ws.numel() * 4, b_pool.data_ptr(), (const float*)scaling.data_ptr(), lb.ids, lb.cu,
                                   y2.data_ptr(), out.data_ptr(), lb.batch, lb.max_seqlen_q, lb.total_q, (int)b_pool.size(0), (int)y2.size(1), (int)k,
                                   (int)b_pool.size(2), dtype_code(y2), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// ---- AWQ quantisation: group quantiser + packer and clip search, one launch each ----
std::tuple<c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>, c10::optional<torch::Tensor>,
           c10::optional<torch::Tensor>>
quantize_pack(torch::Tensor w, c10::optional<torch::Tensor> col_scale, c10::optional<torch::Tensor> clip_max, int64_t n_bit, std::string layout,
              bool want_fake, bool want_scales, bool want_zeros, bool want_qweight) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && (w.stride(1) == 1 || w.size(1) <= 1),
              "awq_inference_engine: quantize_pack: w must be a [N, K] GPU tensor with a contiguous last dimension");
  TORCH_CHECK(layout == "cdna4" || layout == "v2", "quantize_pack: layout must be \"cdna4\" or \"v2\"");
  const int code = dtype_code(w);
  const int64_t n = w.size(0), k = w.size(1);
  TORCH_CHECK(k >= 128 && k % 128 == 0, "quantize_pack: in_features must be a multiple of 128");
  const int64_t g = k / 128, gpad = (g + 7) / 8 * 8;
  auto in = [&](const c10::optional<torch::Tensor>& t, int64_t numel, const char* name) -> void* {
    if (!t.has_value()) return nullptr;
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->scalar_type() == w.scalar_type() && t->numel() == numel && t->device() == w.device(),
                "quantize_pack: ", name, " must be a contiguous GPU tensor of w's dtype and its documented size");
    return t->data_ptr();
  };
  void* cs = in(col_scale, k, "col_scale");
  void* cm = in(clip_max, n * g, "clip_max");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(w.device());
  c10::optional<torch::Tensor> fake, scales, szeros, zeros, qweight;
  if (want_fake) fake = torch::empty({n, k}, w.options());
  if (want_scales) scales = torch::empty({gpad, n}, w.options()), szeros = torch::empty({gpad, n}, w.options());
  if (want_zeros) zeros = torch::empty({n, g}, w.options());
  if (want_qweight) {
    TORCH_CHECK(n % 4 == 0, "quantize_pack: a packed output needs out_features % 8 == 0 (v2) or % 16 == 0 (cdna4)");
    qweight = torch::empty({n / 4, k}, w.options().dtype(at::kShort));
  }
  auto ptr = [](const c10::optional<torch::Tensor>& t) -> void* { return t.has_value() ? t->data_ptr() : nullptr; };
  const int64_t ldw = n > 1 ? w.stride(0) : k;
  raise_on(awq_quantize_group(w.data_ptr(), (long)ldw, cs, cm, ptr(fake), ptr(scales), ptr(szeros), ptr(zeros), ptr(qweight),
                              layout == "cdna4" ? AWQ_QWEIGHT_CDNA4 : AWQ_QWEIGHT_V2, (int)n, (int)k, 128, (int)n_bit, code,
                              (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return std::make_tuple(fake, scales, szeros, zeros, qweight);
}

std::tuple<torch::Tensor, torch::Tensor, c10::optional<torch::Tensor>> clip_search(torch::Tensor w, torch::Tensor x, int64_t n_bit, int64_t n_grid,
                                                                                  int64_t n_steps, bool return_err) {
  TORCH_CHECK(w.is_cuda() && w.dim() == 2 && (w.stride(1) == 1 || w.size(1) <= 1) && x.is_cuda() && x.dim() == 2 &&
                  (x.stride(1) == 1 || x.size(1) <= 1) && x.size(1) == w.size(1) && x.scalar_type() == w.scalar_type() && x.device() == w.device(),
              "awq_inference_engine: clip_search: w [N, K] and x [S, K] must be GPU tensors of one dtype and device with contiguous last dimensions");
  const int code = dtype_code(w);
  const int64_t n = w.size(0), k = w.size(1), s = x.size(0);
  TORCH_CHECK(k >= 128 && k % 128 == 0 && s >= 1 && n >= 1, "clip_search: in_features must be a multiple of 128 and there must be rows and tokens");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(w.device());
  torch::Tensor best = torch::empty({n, k / 128}, w.options());
  torch::Tensor idx = torch::empty({n, k / 128}, w.options().dtype(at::kInt));
  c10::optional<torch::Tensor> err;
  if (return_err) err = torch::empty({n, k / 128, n_steps}, w.options().dtype(at::kFloat));
  raise_on(awq_clip_search(w.data_ptr(), (long)(n > 1 ? w.stride(0) : k), x.data_ptr(), (long)(s > 1 ? x.stride(0) : k), best.data_ptr(),
                           (int*)idx.data_ptr(), err.has_value() ? (float*)err->data_ptr() : nullptr, (int)n, (int)k, (int)s, 128, (int)n_bit,
                           (int)n_grid, (int)n_steps, code, (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return std::make_tuple(best, idx, err);
}

// ---- W3 ("w3c" tiles, bf16): pack from logical integers, and WQLinear.forward for w_bit = 3 ----
torch::Tensor pack_w3(torch::Tensor q_u8) {
  TORCH_CHECK(q_u8.is_cuda() && q_u8.is_contiguous() && q_u8.scalar_type() == at::kByte && q_u8.dim() == 2);
  const int64_t n = q_u8.size(0), k = q_u8.size(1);
  TORCH_CHECK(n % 16 == 0 && k % 128 == 0, "w3c tiles need n % 16 == 0 and k % 128 == 0");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q_u8.device());
  at::Tensor out = torch::empty({n / 4, k * 3 / 4}, q_u8.options().dtype(at::kShort));
  raise_on(awq_pack_w3(q_u8.data_ptr(), out.data_ptr(), (int)n, (int)k,
                       (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

torch::Tensor forward_w3(torch::Tensor in_feats, torch::Tensor kernel, torch::Tensor scales, torch::Tensor zeros,
                         torch::Tensor sz_packed, c10::optional<torch::Tensor> bias) {
  check_inputs(in_feats, kernel, scales, zeros);
  TORCH_CHECK(in_feats.scalar_type() == at::kBFloat16 || in_feats.scalar_type() == at::kHalf, "the W3 path is defined for bfloat16 / float16");
  TORCH_CHECK(sz_packed.is_cuda() && sz_packed.is_contiguous() && sz_packed.scalar_type() == at::kInt);
  const int64_t n = kernel.size(0) * 4, k = in_feats.size(-1);
  TORCH_CHECK(k > 0 && in_feats.numel() % k == 0 && kernel.numel() == n / 4 * (k * 3 / 4), "qweight must be int16 [n/4, 3k/4]");
  TORCH_CHECK(sz_packed.numel() == n * (k / 128), "sz_packed must be int32 [n/16, k/128, 16]");
  const int64_t m = in_feats.numel() / k;
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = n;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  if (m == 0) return out;
  const void* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() && bias->scalar_type() == in_feats.scalar_type() && bias->numel() == n);
    bp = bias->data_ptr();
  }
  const size_t wsb = awq_w3a16_forward_workspace_bytes((int)m, (int)n, (int)k);
  at::Tensor ws;
  if (wsb) ws = torch::empty({(int64_t)wsb}, in_feats.options().dtype(at::kByte));
  raise_on(awq_w3a16_forward(in_feats.data_ptr(), kernel.data_ptr(), scales.data_ptr(), zeros.data_ptr(), sz_packed.data_ptr(),
                             bp, out.data_ptr(), (int)m, (int)n, (int)k, 128, dtype_code(in_feats), wsb ? ws.data_ptr() : nullptr, wsb,
                             (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// QuantLlamaMLP's gate/up + SiLU*mul in one launch (tinychat/modules/fused_mlp.py:36-83), decode rows only
torch::Tensor mlp_gate_up_cdna4(torch::Tensor in_feats, torch::Tensor kernel_gate_up, torch::Tensor sz_packed) {
  TORCH_CHECK(in_feats.is_cuda() && kernel_gate_up.is_cuda() && sz_packed.is_cuda());
  TORCH_CHECK(in_feats.is_contiguous() && kernel_gate_up.is_contiguous() && sz_packed.is_contiguous());
  TORCH_CHECK((in_feats.scalar_type() == at::kBFloat16 || in_feats.scalar_type() == at::kHalf) &&
              kernel_gate_up.scalar_type() == at::kShort && sz_packed.scalar_type() == at::kInt);
  const int64_t n2 = kernel_gate_up.size(0) * 4, k = in_feats.size(-1);
  TORCH_CHECK(k > 0 && in_feats.numel() % k == 0 && kernel_gate_up.numel() == n2 / 4 * k);
  TORCH_CHECK(sz_packed.numel() == n2 * (k / 128), "sz_packed must be int32 [n2/16, k/128, 16]");
  const int64_t m = in_feats.numel() / k;
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = n2 / 2;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  raise_on(awq_w4a16_mlp_gate_up_cdna4(in_feats.data_ptr(), kernel_gate_up.data_ptr(), sz_packed.data_ptr(), out.data_ptr(),
                                       (int)m, (int)n2, (int)k, 128, dtype_code(in_feats),
                                       (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// FTLlamaRMSNorm (tinychat/modules/fused_norm.py:7-21 -> layernorm.cu:39-61) fused in front of the decode GEMV: x is the
// UN-normalised activation, gamma the norm weight [k]; <= 4 rows.  fused_gate_up: kernel = stacked [gate; up], out [.., n/2].
// FTLlamaRMSNorm.forward for any row count (tinychat/modules/fused_norm.py:16-21 -> layernorm_forward_cuda): one launch
torch::Tensor rmsnorm(torch::Tensor in_feats, torch::Tensor gamma, double eps) {
  TORCH_CHECK(in_feats.is_cuda() && gamma.is_cuda() && in_feats.is_contiguous() && gamma.is_contiguous());
  TORCH_CHECK((in_feats.scalar_type() == at::kBFloat16 || in_feats.scalar_type() == at::kHalf) && gamma.scalar_type() == in_feats.scalar_type());
  const int64_t k = in_feats.size(-1);
  TORCH_CHECK(k > 0 && gamma.numel() == k);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty_like(in_feats);
  if (in_feats.numel() == 0) return out;
  raise_on(awq_rmsnorm(in_feats.data_ptr(), gamma.data_ptr(), (float)eps, out.data_ptr(), (int)(in_feats.numel() / k), (int)k, dtype_code(in_feats),
                       (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// layernorm_forward_cuda(x, weight, out, eps) (awq/kernels/csrc/layernorm/layernorm.cu, called by tinychat's FTLlamaRMSNorm,
// modules/fused_norm.py:18, and llama.py:35): the same RMSNorm launch as rmsnorm(), written into the caller's `out`.
void layernorm_forward_cuda(torch::Tensor x, torch::Tensor weight, torch::Tensor out, double eps) {
  TORCH_CHECK(x.is_cuda() && weight.is_cuda() && out.is_cuda(), "layernorm_forward_cuda: tensors must live on the GPU");
  TORCH_CHECK(x.is_contiguous() && weight.is_contiguous() && out.is_contiguous(), "layernorm_forward_cuda: tensors must be contiguous");
  TORCH_CHECK((x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kHalf) && weight.scalar_type() == x.scalar_type() &&
                  out.scalar_type() == x.scalar_type(),
              "layernorm_forward_cuda: float16 / bfloat16 x, weight and out of one dtype are supported");
  const int64_t k = x.size(-1);
  TORCH_CHECK(k > 0 && weight.numel() == k && out.sizes() == x.sizes(), "layernorm_forward_cuda: shape mismatch");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(x.device());
  if (x.numel() == 0) return;
  raise_on(awq_rmsnorm(x.data_ptr(), weight.data_ptr(), (float)eps, out.data_ptr(), (int)(x.numel() / k), (int)k, dtype_code(x),
                       (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
}

// single_query_attention (awq/kernels/csrc/attention/ft_attention.cpp:112-185): one decode step over the FT KV cache
// (csrc/awq_attn_cdna4.hip).  Same shape checks as the reference, except that the batch may be smaller than the cache's
// (tinychat allocates the caches for max_batch_size) and q, k, v keep batch strides of their own.
torch::Tensor single_query_attention(const torch::Tensor q, const torch::Tensor k, const torch::Tensor v, torch::Tensor k_cache,
                                     torch::Tensor v_cache, c10::optional<const torch::Tensor> length_per_sample_,
                                     c10::optional<const torch::Tensor> alibi_slopes_, const int timestep, const int rotary_embedding_dim,
                                     const double rotary_base, const double rotary_scale, const bool neox_rotary_style) {
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&q, &k, &v, &k_cache, &v_cache})
    TORCH_CHECK(t->is_cuda() && t->device() == q.device(), "single_query_attention: tensors must live on the same GPU");
  TORCH_CHECK(q.scalar_type() != at::kFloat,
              "single_query_attention: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "single_query_attention: float16 / bfloat16 only, got ",
              q.scalar_type());
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&k, &v, &k_cache, &v_cache})
    TORCH_CHECK(t->scalar_type() == q.scalar_type(), "single_query_attention: q, k, v and the caches must share one dtype");
  TORCH_CHECK(q.dim() == 3 && k.dim() == 3 && v.dim() == 3 && v_cache.dim() == 4 && k_cache.dim() == 5,
              "single_query_attention: q / k / v [B, heads, Dh], k_cache [B, Hkv, Dh/8, L, 8], v_cache [B, Hkv, L, Dh]");
  const int64_t cache_batch = v_cache.size(0), nheads = q.size(1), nheads_kv = v_cache.size(1), lmax = v_cache.size(2),
                headdim = v_cache.size(3), batch = q.size(0);
  TORCH_CHECK(batch >= 1 && batch <= cache_batch, "single_query_attention: batch ", batch, " exceeds the cache batch ", cache_batch);
  TORCH_CHECK(q.size(2) == headdim, "single_query_attention: q must be [B, H, ", headdim, "]");
  TORCH_CHECK(k.size(0) == batch && k.size(1) == nheads_kv && k.size(2) == headdim, "single_query_attention: k must be [B, Hkv, Dh]");
  TORCH_CHECK(v.size(0) == batch && v.size(1) == nheads_kv && v.size(2) == headdim, "single_query_attention: v must be [B, Hkv, Dh]");
  TORCH_CHECK(k_cache.size(0) == cache_batch && k_cache.size(1) == nheads_kv && k_cache.size(2) == headdim / 8 && k_cache.size(3) == lmax &&
                  k_cache.size(4) == 8 && headdim % 8 == 0,
              "single_query_attention: k_cache must be [B, Hkv, Dh/8, L, 8]");
  TORCH_CHECK(q.stride(2) == 1 && q.stride(1) == headdim);
  TORCH_CHECK(k.stride(2) == 1 && k.stride(1) == headdim);
  TORCH_CHECK(v.stride(2) == 1 && v.stride(1) == headdim);
  TORCH_CHECK(v_cache.is_contiguous() && k_cache.is_contiguous(), "single_query_attention: the caches must be contiguous");
  const int* lens = nullptr;
  if (length_per_sample_.has_value()) {
    const auto& l = length_per_sample_.value();
    TORCH_CHECK(l.is_cuda() && l.device() == q.device() && l.dim() == 1 && l.size(0) >= batch && l.is_contiguous() && l.scalar_type() == at::kInt,
                "single_query_attention: length_per_sample must be a contiguous int32 [B] tensor on the GPU");
    lens = l.data_ptr<int>();
  }
  const float* slopes = nullptr;
  if (alibi_slopes_.has_value()) {
    const auto& a = alibi_slopes_.value();
    TORCH_CHECK(a.is_cuda() && a.device() == q.device() && a.dim() == 1 && a.size(0) == nheads && a.is_contiguous() &&
                    a.scalar_type() == at::kFloat,
                "single_query_attention: alibi_slopes must be a contiguous float32 [H] tensor on the GPU");
    slopes = a.data_ptr<float>();
  }
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  at::Tensor out = torch::empty({batch, nheads, headdim}, q.options().memory_format(at::MemoryFormat::Contiguous));
  const size_t wsb = awq_attn_decode_workspace_bytes((int)batch, (int)nheads, (int)nheads_kv, (int)headdim, timestep, (int)lmax);
  at::Tensor ws;
  if (wsb) ws = torch::empty({(int64_t)wsb}, q.options().dtype(at::kByte));  // caching allocator: capturable
  raise_on(awq_attn_decode(q.data_ptr(), k.data_ptr(), v.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), lens, slopes, out.data_ptr(),
                           (int)batch, (int)cache_batch, (int)nheads, (int)nheads_kv, (int)headdim, (int)lmax, q.stride(0), k.stride(0),
                           v.stride(0), timestep, rotary_embedding_dim, (float)rotary_base, (float)rotary_scale, neox_rotary_style ? 1 : 0,
                           dtype_code(q), wsb ? ws.data_ptr() : nullptr, wsb,
                           (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// flash_attn_func's forward (tinychat llama.py:218, fused_attn.py:477,539) on the gfx950 prefill kernel (csrc/awq_attn_prefill_cdna4.hip):
// q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh] with contiguous heads and batch / row strides of their own (views of one fused qkv tensor pass
// without a copy); causal is bottom-right aligned.  Returns [B, Sq, H, Dh] contiguous.
torch::Tensor attn_prefill(const torch::Tensor q, const torch::Tensor k, const torch::Tensor v, double softmax_scale, bool causal) {
  TORCH_CHECK(q.scalar_type() != at::kFloat, "attn_prefill: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&q, &k, &v})
    TORCH_CHECK(t->is_cuda() && t->device() == q.device(), "attn_prefill: q, k and v must live on the same GPU");
  TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "attn_prefill: float16 / bfloat16 only, got ", q.scalar_type());
  TORCH_CHECK(k.scalar_type() == q.scalar_type() && v.scalar_type() == q.scalar_type(), "attn_prefill: q, k and v must share one dtype");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "attn_prefill: q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh]");
  const int64_t batch = q.size(0), sq = q.size(1), nheads = q.size(2), headdim = q.size(3), sk = k.size(1), nheads_kv = k.size(2);
  TORCH_CHECK(headdim == 64 || headdim == 128 || (headdim == 72 && !causal), "attn_prefill: head dim ", headdim, causal ? " (causal)" : "",
              " is not supported (supported head dims: 64, 128, and 72 without a causal mask)");
  TORCH_CHECK(k.size(0) == batch && k.size(3) == headdim && v.sizes() == k.sizes(), "attn_prefill: k / v must be [B, Sk, Hkv, ", headdim, "]");
  TORCH_CHECK(batch >= 1 && sq >= 1 && sk >= 1 && nheads_kv >= 1 && nheads % nheads_kv == 0,
              "attn_prefill: empty tensors are not supported and H must be a multiple of Hkv");
  TORCH_CHECK(!causal || sq <= sk, "attn_prefill: causal attention needs seqlen_q <= seqlen_k, got ", sq, " > ", sk);
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&q, &k, &v})
    TORCH_CHECK(t->stride(3) == 1 && t->stride(2) == headdim,
                "attn_prefill: the heads of q / k / v must be contiguous (stride(3) == 1, stride(2) == Dh); supported head dims: 64, 128, 72 (non-causal)");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  at::Tensor out = torch::empty({batch, sq, nheads, headdim}, q.options().memory_format(at::MemoryFormat::Contiguous));
  raise_on(awq_attn_prefill(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), (int)batch, (int)sq, (int)sk, (int)nheads, (int)nheads_kv,
                            (int)headdim, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), (float)softmax_scale,
                            causal ? 1 : 0, dtype_code(q), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// The caches of tinychat's QuantLlamaAttentionFused (fused_attn.py:197-224): v_cache [Bc, Hkv, Lmax, Dh], k_cache [Bc, Hkv, Dh/8, Lmax, 8].
static void check_ft_caches(const char* who, const torch::Tensor& ref, const torch::Tensor& k_cache, const torch::Tensor& v_cache) {
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&k_cache, &v_cache}) {
    TORCH_CHECK(t->is_cuda() && t->device() == ref.device(), who, ": the caches must live on the GPU of the input");
    TORCH_CHECK(t->scalar_type() == ref.scalar_type(), who, ": the caches must have the dtype of the input");
  }
  TORCH_CHECK(v_cache.dim() == 4 && k_cache.dim() == 5, who, ": k_cache [Bc, Hkv, Dh/8, Lmax, 8], v_cache [Bc, Hkv, Lmax, Dh]");
  const int64_t headdim = v_cache.size(3);
  TORCH_CHECK(headdim == 64 || headdim == 128, who, ": head dim ", headdim, " is not supported (supported head dims: 64, 128)");
  TORCH_CHECK(k_cache.size(0) == v_cache.size(0) && k_cache.size(1) == v_cache.size(1) && k_cache.size(2) == headdim / 8 &&
                  k_cache.size(3) == v_cache.size(2) && k_cache.size(4) == 8,
              who, ": k_cache must be [Bc, Hkv, Dh/8, Lmax, 8] for v_cache [Bc, Hkv, Lmax, Dh]");
  TORCH_CHECK(v_cache.is_contiguous() && k_cache.is_contiguous(), who, ": the caches must be contiguous");
}

// rope_kv_store(qkv, freqs, k_cache, v_cache, start_pos, nheads, nheads_kv) -> q_out: the prompt side of QuantLlamaAttentionFused.forward
// before the attention (fused_attn.py:248-267, 439-454) in one launch (csrc/awq_attn_chunk_cdna4.hip).  qkv [B, S, (H + 2 Hkv) Dh] with a
// unit last stride (a slice of a wider buffer passes), freqs fp32 with last dim rot_dim and B * S * rot_dim angles.  Returns the rotated
// q [B, S, H, Dh] contiguous; the rotated k and v are written into the caches at positions start_pos .. start_pos + S - 1.
torch::Tensor rope_kv_store(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache, int64_t start_pos,
                            int64_t nheads, int64_t nheads_kv) {
  TORCH_CHECK(qkv.scalar_type() != at::kFloat, "rope_kv_store: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(qkv.is_cuda() && freqs.is_cuda() && freqs.device() == qkv.device(), "rope_kv_store: tensors must live on the same GPU");
  TORCH_CHECK(qkv.scalar_type() == at::kHalf || qkv.scalar_type() == at::kBFloat16, "rope_kv_store: float16 / bfloat16 only, got ", qkv.scalar_type());
  TORCH_CHECK(freqs.scalar_type() == at::kFloat, "rope_kv_store: freqs must be float32");
  check_ft_caches("rope_kv_store", qkv, k_cache, v_cache);
  TORCH_CHECK(qkv.dim() == 3 && freqs.dim() >= 1, "rope_kv_store: qkv must be [B, S, (H + 2 Hkv) * Dh]");
  const int64_t batch = qkv.size(0), seqlen = qkv.size(1), cache_batch = v_cache.size(0), lmax = v_cache.size(2), headdim = v_cache.size(3),
                rot = freqs.size(-1);
  TORCH_CHECK(batch >= 1 && seqlen >= 1 && nheads >= 1 && nheads_kv == v_cache.size(1) && qkv.size(2) == (nheads + 2 * nheads_kv) * headdim,
              "rope_kv_store: qkv must be [B, S, (H + 2 Hkv) * Dh] with the caches' Hkv and Dh");
  TORCH_CHECK(batch <= cache_batch, "rope_kv_store: batch ", batch, " exceeds the cache batch ", cache_batch);
  TORCH_CHECK(start_pos >= 0 && start_pos + seqlen <= lmax, "rope_kv_store: positions ", start_pos, " .. ", start_pos + seqlen,
              " do not fit the cache of ", lmax, " (no wrap on the prompt side)");
  TORCH_CHECK(rot >= 16 && rot % 16 == 0 && rot <= headdim && freqs.numel() >= batch * seqlen * rot,
              "rope_kv_store: freqs must hold B * S * rot_dim angles with rot_dim % 16 == 0 and rot_dim <= head dim");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(qkv.device());
  // the kernel reads 16 bytes at a time: a view whose last stride is not 1, or whose strides / base are not 16-byte multiples, is copied once
  at::Tensor x = qkv;
  if (x.stride(2) != 1 || x.stride(0) % 8 || x.stride(1) % 8 || (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15)) x = qkv.contiguous();
  at::Tensor fr = freqs.is_contiguous() && (reinterpret_cast<uintptr_t>(freqs.data_ptr()) & 15) == 0 ? freqs : freqs.contiguous().clone();
  at::Tensor q_out = torch::empty({batch, seqlen, nheads, headdim}, qkv.options().requires_grad(false).memory_format(at::MemoryFormat::Contiguous));
  raise_on(awq_rope_kv_store(x.data_ptr(), fr.data_ptr<float>(), q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), (int)batch,
                             (int)cache_batch, (int)seqlen, (int)nheads, (int)nheads_kv, (int)headdim, (int)rot, (int)lmax, (int)start_pos,
                             x.stride(0), x.stride(1), dtype_code(x), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return q_out;
}

// attn_prefill_ftcache(q, k_cache, v_cache, kv_start, seqlen_k, softmax_scale, causal) -> out: attn_prefill with K / V read from the FT
// caches, key j = cache position kv_start + j (csrc/awq_attn_prefill_cdna4.hip).  q [B, Sq, H, Dh] with contiguous heads and batch / row
// strides of its own; returns [B, Sq, H, Dh] contiguous, bit-identical to attn_prefill on the gathered keys and values.
torch::Tensor attn_prefill_ftcache(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, int64_t kv_start,
                                   int64_t seqlen_k, double softmax_scale, bool causal) {
  TORCH_CHECK(q.scalar_type() != at::kFloat, "attn_prefill_ftcache: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(q.is_cuda(), "attn_prefill_ftcache: q must live on the GPU");
  TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "attn_prefill_ftcache: float16 / bfloat16 only, got ", q.scalar_type());
  check_ft_caches("attn_prefill_ftcache", q, k_cache, v_cache);
  TORCH_CHECK(q.dim() == 4, "attn_prefill_ftcache: q [B, Sq, H, Dh]");
  const int64_t batch = q.size(0), sq = q.size(1), nheads = q.size(2), headdim = q.size(3), cache_batch = v_cache.size(0),
                nheads_kv = v_cache.size(1), lmax = v_cache.size(2);
  TORCH_CHECK(headdim == v_cache.size(3), "attn_prefill_ftcache: q has head dim ", headdim, ", the caches ", v_cache.size(3));
  TORCH_CHECK(batch >= 1 && sq >= 1 && seqlen_k >= 1 && nheads_kv >= 1 && nheads % nheads_kv == 0,
              "attn_prefill_ftcache: empty tensors are not supported and H must be a multiple of Hkv");
  TORCH_CHECK(batch <= cache_batch, "attn_prefill_ftcache: batch ", batch, " exceeds the cache batch ", cache_batch);
  TORCH_CHECK(kv_start >= 0 && kv_start + seqlen_k <= lmax, "attn_prefill_ftcache: keys ", kv_start, " .. ", kv_start + seqlen_k,
              " do not lie in the cache of ", lmax);
  TORCH_CHECK(!causal || sq <= seqlen_k, "attn_prefill_ftcache: causal attention needs seqlen_q <= seqlen_k, got ", sq, " > ", seqlen_k);
  TORCH_CHECK(q.stride(3) == 1 && q.stride(2) == headdim, "attn_prefill_ftcache: the heads of q must be contiguous (stride(3) == 1, stride(2) == Dh)");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  at::Tensor out = torch::empty({batch, sq, nheads, headdim}, q.options().memory_format(at::MemoryFormat::Contiguous));
  raise_on(awq_attn_prefill_ftcache(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), (int)batch, (int)cache_batch, (int)sq,
                                    (int)kv_start, (int)seqlen_k, (int)nheads, (int)nheads_kv, (int)headdim, (int)lmax, q.stride(0), q.stride(1),
                                    (float)softmax_scale, causal ? 1 : 0, dtype_code(q),
                                    (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// attn_splitkv(q, k, v, softmax_scale, causal) -> out: attn_prefill's arguments and result on the split-KV kernel pair where
// awq_attn_splitkv_plan splits (few query rows over a long history: csrc/awq_attn_splitkv_cdna4.hip), on the one-pass kernel otherwise
// (then bit-identical to attn_prefill).  The fp32 partials live in a buffer of torch's caching allocator: capturable.
torch::Tensor attn_splitkv(const torch::Tensor q, const torch::Tensor k, const torch::Tensor v, double softmax_scale, bool causal) {
  TORCH_CHECK(q.scalar_type() != at::kFloat, "attn_splitkv: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&q, &k, &v})
    TORCH_CHECK(t->is_cuda() && t->device() == q.device(), "attn_splitkv: q, k and v must live on the same GPU");
  TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, "attn_splitkv: float16 / bfloat16 only, got ", q.scalar_type());
  TORCH_CHECK(k.scalar_type() == q.scalar_type() && v.scalar_type() == q.scalar_type(), "attn_splitkv: q, k and v must share one dtype");
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4, "attn_splitkv: q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh]");
  const int64_t batch = q.size(0), sq = q.size(1), nheads = q.size(2), headdim = q.size(3), sk = k.size(1), nheads_kv = k.size(2);
  TORCH_CHECK(headdim == 64 || headdim == 128 || (headdim == 72 && !causal), "attn_splitkv: head dim ", headdim, causal ? " (causal)" : "",
              " is not supported (supported head dims: 64, 128, and 72 without a causal mask)");
  TORCH_CHECK(k.size(0) == batch && k.size(3) == headdim && v.sizes() == k.sizes(), "attn_splitkv: k / v must be [B, Sk, Hkv, ", headdim, "]");
  TORCH_CHECK(batch >= 1 && sq >= 1 && sk >= 1 && nheads_kv >= 1 && nheads % nheads_kv == 0,
              "attn_splitkv: empty tensors are not supported and H must be a multiple of Hkv");
  TORCH_CHECK(!causal || sq <= sk, "attn_splitkv: causal attention needs seqlen_q <= seqlen_k, got ", sq, " > ", sk);
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&q, &k, &v})
    TORCH_CHECK(t->stride(3) == 1 && t->stride(2) == headdim,
                "attn_splitkv: the heads of q / k / v must be contiguous (stride(3) == 1, stride(2) == Dh); supported head dims: 64, 128, 72 (non-causal)");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  at::Tensor out = torch::empty({batch, sq, nheads, headdim}, q.options().memory_format(at::MemoryFormat::Contiguous));
  const size_t wsb = awq_attn_splitkv_workspace_bytes((int)batch, (int)nheads, (int)nheads_kv, (int)headdim, (int)sq, (int)sk, causal ? 1 : 0);
  at::Tensor ws;
  if (wsb) ws = torch::empty({(int64_t)wsb}, q.options().dtype(at::kByte));  // caching allocator: capturable
  raise_on(awq_attn_splitkv(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), (int)batch, (int)sq, (int)sk, (int)nheads, (int)nheads_kv,
                            (int)headdim, q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), (float)softmax_scale,
                            causal ? 1 : 0, dtype_code(q), wsb ? ws.data_ptr() : nullptr, wsb,
                            (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// (splits, chunk) of awq_attn_splitkv_plan; splits == 1: the one-pass kernel serves.  Host only.
std::tuple<int64_t, int64_t> attn_splitkv_plan(int64_t batch, int64_t nheads, int64_t nheads_kv, int64_t head_dim, int64_t seqlen_q,
                                               int64_t seqlen_k, bool causal) {
  int splits = 1, chunk = 0;
  raise_on(awq_attn_splitkv_plan((int)batch, (int)nheads, (int)nheads_kv, (int)head_dim, (int)seqlen_q, (int)seqlen_k, causal ? 1 : 0, &splits,
                                 &chunk));
  return {splits, chunk};
}

// ---- The natural-layout KV cache family (include/awq_cdna4.h): the rope + store bindings and the device-length attention bindings over
//      dense caches [Bc, Lmax, Hkv, Dh] or pools [num_pages, page_size, Hkv, Dh] with a block table, T or FP8 (csrc/awq_kv8.hpp: codes as
//      float8_e4m3fn or uint8, scales [.., Hkv] float32).  One description of the caches, one store and one attention implementation. ----
static bool is_kv8_code(const torch::Tensor& t) { return t.scalar_type() == at::kFloat8_e4m3fn || t.scalar_type() == at::kByte; }

static void check_seqlens(const char* who, const char* name, const torch::Tensor& t, const torch::Tensor& ref, int64_t batch) {
  TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), who, ": ", name, " must live on the GPU of the input (it is read by the kernel only)");
  TORCH_CHECK(t.scalar_type() == at::kInt && t.dim() == 1 && t.size(0) == batch && t.is_contiguous(), who, ": ", name,
              " must be a contiguous int32 [B] tensor");
}

// where K / V of one call live: k_scale set = FP8, block_table set = pools
struct KvTensors {
  const torch::Tensor& k;
  const torch::Tensor& v;
  const torch::Tensor* k_scale;
  const torch::Tensor* v_scale;
  const torch::Tensor* block_table;
};

// Describe the caches or pools: devices, dtypes (ref's, or codes), one shape with contiguous heads, the scales of that shape, the table
// [>= batch, pages_per_seq].  contiguous: the dense store entries take no strides.  ref_name: how the messages call the tensor `ref`.
static void check_kv(const char* who, const KvTensors& kv, const torch::Tensor& ref, const char* ref_name, int64_t batch, bool contiguous) {
  const bool fp8 = kv.k_scale != nullptr, paged = kv.block_table != nullptr;
  const char* name[2] = {paged ? "k_pool" : "k_cache", paged ? "v_pool" : "v_cache"};
  const char* sname[2] = {"k_scale", "v_scale"};
  const char* layout = paged ? "[num_pages, page_size, Hkv, Dh]" : "[Bc, Lmax, Hkv, Dh]";
  const torch::Tensor* tensors[2] = {&kv.k, &kv.v};
  const torch::Tensor* scales[2] = {kv.k_scale, kv.v_scale};
  for (int i = 0; i < 2; ++i) {
    const torch::Tensor& t = *tensors[i];
    TORCH_CHECK(t.is_cuda() && t.device() == ref.device(), who, ": ", name[i], " must live on the GPU of ", ref_name);
    if (fp8) {
      TORCH_CHECK(is_kv8_code(t), who, ": ", name[i], " must be float8_e4m3fn or uint8, got ", t.scalar_type());
    } else {
      TORCH_CHECK(t.scalar_type() == ref.scalar_type(), who, ": ", name[i], " must have the dtype of ", ref_name, ", got ", t.scalar_type());
    }
    TORCH_CHECK(t.dim() == 4 && t.stride(3) == 1 && t.stride(2) == t.size(3) && (!contiguous || t.is_contiguous()), who, ": ", name[i], " must be ",
                contiguous ? "contiguous " : "", layout, contiguous ? "" : " with contiguous heads (stride(3) == 1, stride(2) == Dh)");
  }
  TORCH_CHECK(kv.k.sizes() == kv.v.sizes(), who, ": ", name[0], " and ", name[1], " must have one shape ", layout);
  if (paged)
    TORCH_CHECK(kv.k.size(0) >= 1 && kv.k.size(1) >= 64 && kv.k.size(1) % 64 == 0, who, ": page size ", kv.k.size(1),
                " is not supported (a multiple of 64, at least 64) or the pool is empty");
  for (int i = 0; fp8 && i < 2; ++i) {
    const torch::Tensor& s = *scales[i];
    TORCH_CHECK(s.is_cuda() && s.device() == ref.device(), who, ": ", sname[i], " must live on the GPU of ", ref_name);
    TORCH_CHECK(s.scalar_type() == at::kFloat, who, ": ", sname[i], " must be float32, got ", s.scalar_type());
    TORCH_CHECK(s.dim() == 3 && s.size(0) == kv.k.size(0) && s.size(1) == kv.k.size(1) && s.size(2) == kv.k.size(2) && s.stride(2) == 1 &&
                    (!contiguous || s.is_contiguous()),
                who, ": ", sname[i], " must be ", contiguous ? "contiguous " : "", paged ? "[num_pages, page_size, Hkv]" : "[Bc, Lmax, Hkv]", " of ",
                name[i], contiguous ? "" : " with a unit last stride");
  }
  if (paged) {
    const torch::Tensor& bt = *kv.block_table;
    TORCH_CHECK(bt.is_cuda() && bt.device() == ref.device(), who, ": block_table must live on the GPU of ", ref_name,
                " (it is read by the kernel only)");
    TORCH_CHECK(bt.scalar_type() == at::kInt && bt.dim() == 2 && bt.size(0) >= batch && bt.size(1) >= 1 && bt.stride(1) == 1 &&
                    bt.stride(0) >= bt.size(1),
                who, ": block_table must be an int32 [>= B, pages_per_seq] tensor with a unit last stride");
  }
}

// A packed step (continuous batching, include/awq_cdna4.h "varq"), the optional part of a call's description: the tokens are one flat run
// of rows, sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1, read on the device.  out / q_out may be handed in (a buffer of
// a fixed token budget whose padding rows the launches leave alone); otherwise they are allocated and rows >= cu[B] hold whatever the
// allocator left.  cu == nullptr: the rectangle [B, S].
struct PackedStep {
  const torch::Tensor* cu = nullptr;
  int64_t max_seqlen_q = 0;
  const c10::optional<torch::Tensor>* out = nullptr;
  bool lens_before_step = false;  // attention only
  // attention only, a mixed step (attn_varq and its siblings): the split pair takes the sequences with at most split_seqlen_q new tokens over
  // at least split_min_keys keys.  split_seqlen_q < 0: not a mixed call
  int64_t split_seqlen_q = -1, split_min_keys = 0;
  // a mixed step with a sliding window (attn_varq_window and its siblings): a row attends its own key and the window_left keys before it.
  // window_left < 0: no window
  int64_t window_left = -1;
  // a windowed step whose logits are capped (attn_varq_softcap and its siblings): cap * tanh(scale * q.k / cap) in front of the mask.
  // capped: the call goes to the *_softcap entries, which hand softcap = 0 to the *_window ones
  bool capped = false;
  double softcap = 0.0;
};

static void check_cu_seqlens(const char* who, const torch::Tensor& cu, const torch::Tensor& ref, int64_t max_seqlen_q) {
  TORCH_CHECK(cu.is_cuda() && cu.device() == ref.device(), who, ": cu_seqlens_q must live on the GPU of the input (it is read by the kernel only)");
  TORCH_CHECK(cu.scalar_type() == at::kInt && cu.dim() == 1 && cu.size(0) >= 2 && cu.is_contiguous(), who,
              ": cu_seqlens_q must be a contiguous int32 [B + 1] tensor");
  TORCH_CHECK(cu.size(0) - 1 <= 65535, who, ": batch ", cu.size(0) - 1, " exceeds 65535");
  TORCH_CHECK(max_seqlen_q >= 1, who, ": max_seqlen_q must be at least 1");
}

static at::Tensor packed_out(const char* who, const char* name, const c10::optional<torch::Tensor>& given, const torch::Tensor& ref, int64_t total,
                             int64_t nheads, int64_t headdim) {
  if (!given.has_value()) return torch::empty({total, nheads, headdim}, ref.options().requires_grad(false).memory_format(at::MemoryFormat::Contiguous));
  const torch::Tensor& o = *given;
  TORCH_CHECK(o.is_cuda() && o.device() == ref.device() && o.scalar_type() == ref.scalar_type() && o.dim() == 3 && o.size(0) == total &&
                  o.size(1) == nheads && o.size(2) == headdim && o.is_contiguous(),
              who, ": ", name, " must be a contiguous [total_q, H, Dh] tensor of the input's dtype on its GPU");
  return o;
}

// The store bindings.  cache_seqlens == nullptr: the host position start_pos, freqs holds the call's B * S * rot_dim angles (copied when
// misaligned).  Otherwise each sequence's position is read on the device and freqs is the model's whole table [P, rot_dim] (not copied:
// a misaligned one is refused).  step: qkv is the packed tokens [total_q, ..] (device positions only).  One launch
// (csrc/awq_attn_chunk_cdna4.hip, csrc/awq_attn_kv8_cdna4.hip).
// the per-head q/k RMSNorm of the *_qknorm bindings: gammas float32 [Dh] on the GPU of qkv (Gemma-3's 1 + w is formed in fp32)
struct QkNorm {
  const torch::Tensor* q_gamma;
  const torch::Tensor* k_gamma;
  double eps;
};

// norm: the entry's _qknorm sibling serves -- q and k heads are RMS-normalised over Dh before the rotation, in the same launch.
static torch::Tensor rope_store_impl(const char* who, const torch::Tensor& qkv, const torch::Tensor& freqs, const KvTensors& kv,
                                     const torch::Tensor* cache_seqlens, int64_t start_pos, int64_t nheads, int64_t nheads_kv,
                                     const PackedStep& step = {}, const QkNorm* norm = nullptr) {
  const bool fp8 = kv.k_scale != nullptr, paged = kv.block_table != nullptr, devlen = cache_seqlens != nullptr, packed = step.cu != nullptr;
  TORCH_CHECK(qkv.scalar_type() != at::kFloat, who, ": float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(qkv.is_cuda() && freqs.is_cuda() && freqs.device() == qkv.device(), who, ": tensors must live on the same GPU");
  TORCH_CHECK(qkv.scalar_type() == at::kHalf || qkv.scalar_type() == at::kBFloat16, who, ": float16 / bfloat16 only, got ", qkv.scalar_type());
  if (devlen) {
    TORCH_CHECK(freqs.scalar_type() == at::kFloat && freqs.dim() == 2 && freqs.is_contiguous() &&
                    (reinterpret_cast<uintptr_t>(freqs.data_ptr()) & 15) == 0,
                who, ": freqs_table must be a contiguous, 16-byte aligned float32 [P, rot_dim] tensor (the whole angle table; it is not copied)");
  } else {
    TORCH_CHECK(freqs.scalar_type() == at::kFloat, who, ": freqs must be float32");
  }
  if (packed) {
    TORCH_CHECK(qkv.dim() == 2, who, ": qkv must be the packed tokens [total_q, (H + 2 Hkv) * Dh]");
    check_cu_seqlens(who, *step.cu, qkv, step.max_seqlen_q);
  } else {
    TORCH_CHECK(qkv.dim() == 3 && freqs.dim() >= 1, who, ": qkv must be [B, S, (H + 2 Hkv) * Dh]");
  }
  // the rectangle [batch, seqlen], or total packed rows of batch sequences that bring at most seqlen each
  const int64_t batch = packed ? step.cu->size(0) - 1 : qkv.size(0), seqlen = packed ? step.max_seqlen_q : qkv.size(1), total = qkv.size(0);
  check_kv(who, kv, qkv, "the input", batch, /*contiguous=*/!paged);
  const torch::Tensor &k = kv.k, &v = kv.v;
  const int64_t outer = k.size(0), rows = k.size(1), headdim = k.size(3), rot = freqs.size(-1);
  TORCH_CHECK(headdim == 64 || headdim == 128, who, ": head dim ", headdim, " is not supported (supported head dims: 64, 128)");
  if (packed) {
    TORCH_CHECK(total >= 1 && nheads >= 1 && nheads_kv == k.size(2) && qkv.size(1) == (nheads + 2 * nheads_kv) * headdim, who,
                ": qkv must be [total_q, (H + 2 Hkv) * Dh] with the ", paged ? "pools'" : "caches'", " Hkv and Dh");
  } else {
    TORCH_CHECK(batch >= 1 && seqlen >= 1 && nheads >= 1 && nheads_kv == k.size(2) && qkv.size(2) == (nheads + 2 * nheads_kv) * headdim, who,
                ": qkv must be [B, S, (H + 2 Hkv) * Dh] with the ", paged ? "pools'" : "caches'", " Hkv and Dh");
  }
  TORCH_CHECK(paged || batch <= outer, who, ": batch ", batch, " exceeds the cache batch ", outer);
  if (devlen) {
    TORCH_CHECK(freqs.size(0) >= 1 && rot >= 16 && rot % 16 == 0 && rot <= headdim, who,
                ": freqs_table must be [P >= 1, rot_dim] with rot_dim % 16 == 0 and rot_dim <= head dim");
    check_seqlens(who, "cache_seqlens", *cache_seqlens, qkv, batch);
  } else {
    TORCH_CHECK(start_pos >= 0 && start_pos + seqlen <= rows, who, ": positions ", start_pos, " .. ", start_pos + seqlen,
                " do not fit the cache of ", rows);
    TORCH_CHECK(rot >= 16 && rot % 16 == 0 && rot <= headdim && freqs.numel() >= batch * seqlen * rot, who,
                ": freqs must hold B * S * rot_dim angles with rot_dim % 16 == 0 and rot_dim <= head dim");
  }
  if (norm) {
    for (const torch::Tensor* g : {norm->q_gamma, norm->k_gamma})
      TORCH_CHECK(g->is_cuda() && g->device() == qkv.device() && g->scalar_type() == at::kFloat && g->dim() == 1 && g->size(0) == headdim &&
                      g->is_contiguous() && (reinterpret_cast<uintptr_t>(g->data_ptr()) & 15) == 0,
                  who, ": q_gamma and k_gamma must be contiguous, 16-byte aligned float32 [Dh] tensors on the GPU of qkv");
    TORCH_CHECK(norm->eps >= 0 && std::isfinite(norm->eps), who, ": norm_eps must be finite and >= 0");
  }
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(qkv.device());
  at::Tensor x = qkv;  // rows of a unit stride, every other stride a multiple of 16 bytes
  if (x.stride(-1) != 1 || x.stride(0) % 8 || x.stride(-2) % 8 || (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15)) x = qkv.contiguous();
  at::Tensor fr = devlen || (freqs.is_contiguous() && (reinterpret_cast<uintptr_t>(freqs.data_ptr()) & 15) == 0) ? freqs : freqs.contiguous().clone();
  at::Tensor q_out = packed ? packed_out(who, "q_out", *step.out, qkv, total, nheads, headdim)
                            : torch::empty({batch, seqlen, nheads, headdim},
                                           qkv.options().requires_grad(false).memory_format(at::MemoryFormat::Contiguous));
  void* st = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  void *xp = x.data_ptr(), *qp = q_out.data_ptr(), *kp = k.data_ptr(), *vp = v.data_ptr();
  const float* fp = fr.data_ptr<float>();
  float *ksp = fp8 ? kv.k_scale->data_ptr<float>() : nullptr, *vsp = fp8 ? kv.v_scale->data_ptr<float>() : nullptr;
  const int *pos = devlen ? cache_seqlens->data_ptr<int>() : nullptr, *cup = packed ? step.cu->data_ptr<int>() : nullptr;
  // S: the rectangle's seqlen, or the packed step's bound max_seqlen_q; T: the packed rows
  const int B = (int)batch, S = (int)seqlen, T = (int)total, H = (int)nheads, Hkv = (int)nheads_kv, Dh = (int)headdim, R = (int)rot,
            P = devlen ? (int)freqs.size(0) : 0, dt = dtype_code(x);
  const int64_t bs = x.stride(0), rs = x.stride(-2);
  const float *qg = norm ? norm->q_gamma->data_ptr<float>() : nullptr, *kg = norm ? norm->k_gamma->data_ptr<float>() : nullptr;
  const float eps = norm ? (float)norm->eps : 0.f;
// the entry, or with norm its _qknorm sibling: the same arguments with the gammas and eps directly after the angles
#define AWQ_STORE(entry, ...) raise_on(norm ? entry##_qknorm(xp, fp, qg, kg, eps, __VA_ARGS__) : entry(xp, fp, __VA_ARGS__))
  if (paged) {
    const torch::Tensor& bt = *kv.block_table;
    const int pages = (int)outer, page = (int)rows, pps = (int)bt.size(1);
    const int64_t kps = k.stride(0), krs = k.stride(1), vps = v.stride(0), vrs = v.stride(1);
    if (packed && fp8)
      AWQ_STORE(awq_rope_kv_store_paged_varq_fp8, qp, kp, vp, ksp, vsp, bt.data_ptr<int>(), pos, B, cup, S, T, H, Hkv, Dh, R, P, pages, page,
                                                pps, bt.stride(0), kps, krs, vps, vrs, kv.k_scale->stride(0), kv.k_scale->stride(1),
                                                kv.v_scale->stride(0), kv.v_scale->stride(1), rs, dt, st);
    else if (packed)
      AWQ_STORE(awq_rope_kv_store_paged_varq, qp, kp, vp, bt.data_ptr<int>(), pos, B, cup, S, T, H, Hkv, Dh, R, P, pages, page, pps,
                                            bt.stride(0), kps, krs, vps, vrs, rs, dt, st);
    else if (fp8)
      AWQ_STORE(awq_rope_kv_store_paged_pos_fp8, qp, kp, vp, ksp, vsp, bt.data_ptr<int>(), pos, B, S, H, Hkv, Dh, R, P, pages, page, pps,
                                               bt.stride(0), kps, krs, vps, vrs, kv.k_scale->stride(0), kv.k_scale->stride(1),
                                               kv.v_scale->stride(0), kv.v_scale->stride(1), bs, rs, dt, st);
    else
      AWQ_STORE(awq_rope_kv_store_paged_pos, qp, kp, vp, bt.data_ptr<int>(), pos, B, S, H, Hkv, Dh, R, P, pages, page, pps, bt.stride(0),
                                           kps, krs, vps, vrs, bs, rs, dt, st);
  } else if (packed) {
    if (fp8) AWQ_STORE(awq_rope_kv_store_natural_varq_fp8, qp, kp, vp, ksp, vsp, pos, B, (int)outer, cup, S, T, H, Hkv, Dh, R, (int)rows, P, rs, dt, st);
    else AWQ_STORE(awq_rope_kv_store_natural_varq, qp, kp, vp, pos, B, (int)outer, cup, S, T, H, Hkv, Dh, R, (int)rows, P, rs, dt, st);
  } else if (devlen) {
    if (fp8) AWQ_STORE(awq_rope_kv_store_natural_pos_fp8, qp, kp, vp, ksp, vsp, pos, B, (int)outer, S, H, Hkv, Dh, R, (int)rows, P, bs, rs, dt, st);
    else AWQ_STORE(awq_rope_kv_store_natural_pos, qp, kp, vp, pos, B, (int)outer, S, H, Hkv, Dh, R, (int)rows, P, bs, rs, dt, st);
  } else {
    if (fp8)
      AWQ_STORE(awq_rope_kv_store_natural_fp8, qp, kp, vp, ksp, vsp, B, (int)outer, S, H, Hkv, Dh, R, (int)rows, (int)start_pos, bs, rs, dt, st);
    else AWQ_STORE(awq_rope_kv_store_natural, qp, kp, vp, B, (int)outer, S, H, Hkv, Dh, R, (int)rows, (int)start_pos, bs, rs, dt, st);
  }
#undef AWQ_STORE
  return q_out;
}

// rope_kv_store_natural(qkv, freqs, k_cache, v_cache, start_pos, nheads, nheads_kv) -> q_out: rope_kv_store for the natural-layout caches
// k_cache / v_cache [Bc, Lmax, Hkv, Dh] of tinychat's long-context path (fused_attn.py:527-537).
torch::Tensor rope_kv_store_natural(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache,
                                    int64_t start_pos, int64_t nheads, int64_t nheads_kv) {
  return rope_store_impl("rope_kv_store_natural", qkv, freqs, {k_cache, v_cache, nullptr, nullptr, nullptr}, nullptr, start_pos, nheads, nheads_kv);
}

// ... with k and v quantised per (token, KV head) on their way into the caches.  q_out holds rope_kv_store_natural's bits.
torch::Tensor rope_kv_store_natural_fp8(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache,
                                        torch::Tensor k_scale, torch::Tensor v_scale, int64_t start_pos, int64_t nheads, int64_t nheads_kv) {
  return rope_store_impl("rope_kv_store_natural_fp8", qkv, freqs, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, nullptr, start_pos, nheads,
                         nheads_kv);
}

// rope_kv_store_natural_pos(qkv, freqs_table, k_cache, v_cache, cache_seqlens, nheads, nheads_kv) -> q_out: rope_kv_store_natural with each
// sequence's position read on the device (cache_seqlens int32 [B]) and the angles taken from the whole table freqs_table [P, rot_dim].
torch::Tensor rope_kv_store_natural_pos(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_cache, torch::Tensor v_cache,
                                        const torch::Tensor cache_seqlens, int64_t nheads, int64_t nheads_kv) {
  return rope_store_impl("rope_kv_store_natural_pos", qkv, freqs_table, {k_cache, v_cache, nullptr, nullptr, nullptr}, &cache_seqlens, 0, nheads,
                         nheads_kv);
}

torch::Tensor rope_kv_store_natural_pos_fp8(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_cache, torch::Tensor v_cache,
                                            torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor cache_seqlens, int64_t nheads,
                                            int64_t nheads_kv) {
  return rope_store_impl("rope_kv_store_natural_pos_fp8", qkv, freqs_table, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, &cache_seqlens, 0,
                         nheads, nheads_kv);
}

// rope_kv_store_paged_pos(qkv, freqs_table, k_pool, v_pool, block_table, cache_seqlens, nheads, nheads_kv) -> q_out: rope_kv_store_natural_pos
// writing token s of sequence b at logical position cache_seqlens[b] + s of the pages block_table[b] names.
torch::Tensor rope_kv_store_paged_pos(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_pool, torch::Tensor v_pool,
                                      const torch::Tensor block_table, const torch::Tensor cache_seqlens, int64_t nheads, int64_t nheads_kv) {
  return rope_store_impl("rope_kv_store_paged_pos", qkv, freqs_table, {k_pool, v_pool, nullptr, nullptr, &block_table}, &cache_seqlens, 0, nheads,
                         nheads_kv);
}

torch::Tensor rope_kv_store_paged_pos_fp8(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_pool, torch::Tensor v_pool,
                                          torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor block_table,
                                          const torch::Tensor cache_seqlens, int64_t nheads, int64_t nheads_kv) {
  return rope_store_impl("rope_kv_store_paged_pos_fp8", qkv, freqs_table, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, &cache_seqlens, 0,
                         nheads, nheads_kv);
}

// attn_kvcache[_paged][_kv8](q, caches or pools .., seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale, causal) -> out: the split-KV pair
// with Sk_b = seqlens_k[b] + seqlen_offset read on the device, K / V from the caches or fetched from the pools through the table.  The fp32
// partials live in a buffer of torch's caching allocator, so a graph capture owns them.  one_pass: attn_prefill_kvcache[_kv8] /
// attn_prefill_paged[_kv8], the one-pass prefill kernel under the same lengths -- any seqlen_q, no workspace.  step (one_pass only): q is
// the packed rows [total_q, H, Dh], and the flag lens_before_step stands in the place of seqlen_offset.
static torch::Tensor attn_kvcache_impl(const char* who, const torch::Tensor& q, const KvTensors& kv, const torch::Tensor& seqlens_k,
                                       int64_t max_seqlen_k, int64_t seqlen_offset, double softmax_scale, bool causal, bool one_pass = false,
                                       const PackedStep& step = {}) {
  const bool fp8 = kv.k_scale != nullptr, paged = kv.block_table != nullptr, packed = step.cu != nullptr;
  const bool mixed = packed && step.split_seqlen_q >= 0;
  TORCH_CHECK(q.scalar_type() != at::kFloat, who, ": float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(q.is_cuda(), who, ": q must live on the GPU");
  TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, who, ": float16 / bfloat16 only, got ", q.scalar_type());
  if (packed) {
    TORCH_CHECK(q.dim() == 3 && q.stride(2) == 1 && q.stride(1) == q.size(2), who, ": q [total_q, H, Dh] (packed rows) with contiguous heads is expected");
    check_cu_seqlens(who, *step.cu, q, step.max_seqlen_q);
  } else {
    TORCH_CHECK(q.dim() == 4 && q.stride(3) == 1 && q.stride(2) == q.size(3), who, ": q [B, Sq, H, Dh] with contiguous heads is expected");
  }
  // the rectangle [batch, sq], or total packed rows of batch sequences that bring at most sq each
  const int64_t batch = packed ? step.cu->size(0) - 1 : q.size(0), sq = packed ? step.max_seqlen_q : q.size(1), total = q.size(0),
                nheads = q.size(-2), headdim = q.size(-1);
  if (packed) seqlen_offset = step.lens_before_step ? 1 : 0;
  TORCH_CHECK(headdim == 64 || headdim == 128, who, ": head dim ", headdim, " is not supported (supported head dims: 64, 128)");
  check_kv(who, kv, q, "q", batch, /*contiguous=*/false);
  const torch::Tensor &k = kv.k, &v = kv.v;
  const int64_t outer = k.size(0), rows = k.size(1), nheads_kv = k.size(2), cap = paged ? kv.block_table->size(1) * rows : rows;
  TORCH_CHECK((paged || outer >= batch) && k.size(3) == headdim, who, ": ", paged ? "k_pool / v_pool must be [num_pages, page_size, Hkv, " : "k_cache / v_cache must be [Bc >= B, Lmax, Hkv, ",
              headdim, "]");
  TORCH_CHECK((packed ? total >= 1 : batch >= 1 && sq >= 1) && nheads_kv >= 1 && nheads % nheads_kv == 0, who,
              ": empty tensors are not supported and H must be a multiple of Hkv");
  TORCH_CHECK(one_pass || sq * (nheads / nheads_kv) <= 128, who, ": seqlen_q * (H / Hkv) = ", sq * (nheads / nheads_kv),
              " exceeds 128 (the split kernels serve few query rows; ",
              paged ? "feed a longer prompt in pieces)" : "a prompt goes through the host-length path)");
  TORCH_CHECK(max_seqlen_k >= 1 && max_seqlen_k <= cap, who, ": max_seqlen_k ", max_seqlen_k, " must lie in 1 .. ", cap,
              paged ? " (pages_per_seq * page_size)" : " (the cache length)");
  TORCH_CHECK(seqlen_offset >= 0, who, ": seqlen_offset must not be negative");
  if (mixed)
    TORCH_CHECK(step.split_min_keys >= 1 && step.split_seqlen_q * (nheads / nheads_kv) <= 128, who, ": split_min_keys ", step.split_min_keys,
                " must be at least 1 and split_seqlen_q * (H / Hkv) = ", step.split_seqlen_q * (nheads / nheads_kv), " at most 128");
  const bool windowed = mixed && step.window_left >= 0;
  const int wl = (int)std::min<int64_t>(step.window_left, 0x7FFFFFFF);
  if (windowed) TORCH_CHECK(causal, who, ": a sliding window needs causal = true");
  const bool capped = windowed && step.capped;
  const float scap = (float)step.softcap;
  if (step.capped)
    TORCH_CHECK(windowed && step.softcap >= 0.0 && scap <= 3.4028234663852886e38f, who, ": softcap ", step.softcap,
                " must be finite and not negative (0: no cap)");
  check_seqlens(who, "seqlens_k", seqlens_k, q, batch);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  at::Tensor out = packed ? packed_out(who, "out", *step.out, q, total, nheads, headdim)
                          : torch::empty({batch, sq, nheads, headdim}, q.options().memory_format(at::MemoryFormat::Contiguous));
  const size_t wsb = windowed   ? awq_attn_varq_window_workspace_bytes((int)batch, (int)nheads, (int)nheads_kv, (int)headdim,
                                                                       (int)step.split_seqlen_q, (int)max_seqlen_k, wl)
                     : mixed    ? awq_attn_varq_split_workspace_bytes((int)batch, (int)nheads, (int)nheads_kv, (int)headdim,
                                                                      (int)step.split_seqlen_q, (int)max_seqlen_k)
                     : one_pass ? 0
                                : awq_attn_kvcache_workspace_bytes((int)batch, (int)nheads, (int)nheads_kv, (int)headdim, (int)sq, (int)max_seqlen_k);
  at::Tensor ws = torch::empty({(int64_t)wsb}, q.options().dtype(at::kByte));  // caching allocator: capturable
  void* st = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  void *qp = q.data_ptr(), *kp = k.data_ptr(), *vp = v.data_ptr(), *op = out.data_ptr();
  const float *ksp = fp8 ? kv.k_scale->data_ptr<float>() : nullptr, *vsp = fp8 ? kv.v_scale->data_ptr<float>() : nullptr;
  const int *lens = seqlens_k.data_ptr<int>(), *cup = packed ? step.cu->data_ptr<int>() : nullptr;
  // Sq: the rectangle's seqlen_q, or the packed step's bound max_seqlen_q; T: the packed rows; off: seqlen_offset, or the flag
  const int B = (int)batch, Sq = (int)sq, T = (int)total, H = (int)nheads, Hkv = (int)nheads_kv, Dh = (int)headdim, off = (int)seqlen_offset,
            bound = (int)max_seqlen_k, cz = causal ? 1 : 0, dt = dtype_code(q), L = (int)rows;
  const float scale = (float)softmax_scale;
  const int64_t qbs = q.stride(0), qrs = q.stride(-3), kbs = k.stride(0), krs = k.stride(1), vbs = v.stride(0), vrs = v.stride(1),
                ksbs = fp8 ? kv.k_scale->stride(0) : 0, ksrs = fp8 ? kv.k_scale->stride(1) : 0, vsbs = fp8 ? kv.v_scale->stride(0) : 0,
                vsrs = fp8 ? kv.v_scale->stride(1) : 0;
  const int* btp = paged ? kv.block_table->data_ptr<int>() : nullptr;
  const int pages = (int)outer, page = (int)rows, pps = paged ? (int)kv.block_table->size(1) : 0;
  const int64_t btrs = paged ? kv.block_table->stride(0) : 0;
  if (mixed) {
    const int ssq = (int)step.split_seqlen_q, smk = (int)std::min<int64_t>(step.split_min_keys, 0x7FFFFFFF);
    void* wp = wsb ? ws.data_ptr() : nullptr;
    if (capped && paged && fp8)
      raise_on(awq_attn_paged_varq_softcap_kv8(qp, kp, vp, ksp, vsp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs,
                                               kbs, krs, vbs, vrs, ksbs, ksrs, vsbs, vsrs, scale, cz, dt, ssq, smk, wl, scap, wp, wsb, st));
    else if (capped && paged)
      raise_on(awq_attn_paged_varq_softcap(qp, kp, vp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs, kbs, krs, vbs,
                                           vrs, scale, cz, dt, ssq, smk, wl, scap, wp, wsb, st));
    else if (capped && fp8)
      raise_on(awq_attn_varq_softcap_kv8(qp, kp, vp, ksp, vsp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, ksbs, ksrs,
                                         vsbs, vsrs, scale, cz, dt, ssq, smk, wl, scap, wp, wsb, st));
    else if (capped)
      raise_on(awq_attn_varq_softcap(qp, kp, vp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, scale, cz, dt, ssq, smk,
                                     wl, scap, wp, wsb, st));
    else if (windowed && paged && fp8)
      raise_on(awq_attn_paged_varq_window_kv8(qp, kp, vp, ksp, vsp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs,
                                              kbs, krs, vbs, vrs, ksbs, ksrs, vsbs, vsrs, scale, cz, dt, ssq, smk, wl, wp, wsb, st));
    else if (windowed && paged)
      raise_on(awq_attn_paged_varq_window(qp, kp, vp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs, kbs, krs, vbs,
                                          vrs, scale, cz, dt, ssq, smk, wl, wp, wsb, st));
    else if (windowed && fp8)
      raise_on(awq_attn_varq_window_kv8(qp, kp, vp, ksp, vsp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, ksbs, ksrs,
                                        vsbs, vsrs, scale, cz, dt, ssq, smk, wl, wp, wsb, st));
    else if (windowed)
      raise_on(awq_attn_varq_window(qp, kp, vp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, scale, cz, dt, ssq, smk,
                                    wl, wp, wsb, st));
    else if (paged && fp8)
      raise_on(awq_attn_paged_varq_kv8(qp, kp, vp, ksp, vsp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs, kbs, krs,
                                       vbs, vrs, ksbs, ksrs, vsbs, vsrs, scale, cz, dt, ssq, smk, wp, wsb, st));
    else if (paged)
      raise_on(awq_attn_paged_varq(qp, kp, vp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs,
                                   scale, cz, dt, ssq, smk, wp, wsb, st));
    else if (fp8)
      raise_on(awq_attn_varq_kv8(qp, kp, vp, ksp, vsp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, ksbs, ksrs, vsbs,
                                 vsrs, scale, cz, dt, ssq, smk, wp, wsb, st));
    else
      raise_on(awq_attn_varq(qp, kp, vp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, scale, cz, dt, ssq, smk, wp, wsb,
                             st));
  } else if (packed) {
    if (paged && fp8)
      raise_on(awq_attn_prefill_paged_varq_kv8(qp, kp, vp, ksp, vsp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs,
                                               kbs, krs, vbs, vrs, ksbs, ksrs, vsbs, vsrs, scale, cz, dt, st));
    else if (paged)
      raise_on(awq_attn_prefill_paged_varq(qp, kp, vp, op, btp, B, cup, Sq, T, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qrs, kbs, krs, vbs,
                                           vrs, scale, cz, dt, st));
    else if (fp8)
      raise_on(awq_attn_prefill_kvcache_varq_kv8(qp, kp, vp, ksp, vsp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, ksbs,
                                                 ksrs, vsbs, vsrs, scale, cz, dt, st));
    else
      raise_on(awq_attn_prefill_kvcache_varq(qp, kp, vp, op, B, cup, Sq, T, lens, off, bound, L, H, Hkv, Dh, qrs, kbs, krs, vbs, vrs, scale, cz, dt, st));
  } else if (one_pass) {
    if (paged && fp8)
      raise_on(awq_attn_prefill_paged_kv8(qp, kp, vp, ksp, vsp, op, btp, B, Sq, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qbs, qrs, kbs, krs,
                                          vbs, vrs, ksbs, ksrs, vsbs, vsrs, scale, cz, dt, st));
    else if (paged)
      raise_on(awq_attn_prefill_paged(qp, kp, vp, op, btp, B, Sq, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qbs, qrs, kbs, krs, vbs, vrs,
                                      scale, cz, dt, st));
    else if (fp8)
      raise_on(awq_attn_prefill_kvcache_kv8(qp, kp, vp, ksp, vsp, op, B, Sq, lens, off, bound, L, H, Hkv, Dh, qbs, qrs, kbs, krs, vbs, vrs, ksbs, ksrs,
                                            vsbs, vsrs, scale, cz, dt, st));
    else raise_on(awq_attn_prefill_kvcache(qp, kp, vp, op, B, Sq, lens, off, bound, L, H, Hkv, Dh, qbs, qrs, kbs, krs, vbs, vrs, scale, cz, dt, st));
  } else {
    if (paged && fp8)
      raise_on(awq_attn_kvcache_paged_kv8(qp, kp, vp, ksp, vsp, op, btp, B, Sq, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qbs, qrs, kbs, krs,
                                          vbs, vrs, ksbs, ksrs, vsbs, vsrs, scale, cz, dt, ws.data_ptr(), wsb, st));
    else if (paged)
      raise_on(awq_attn_kvcache_paged(qp, kp, vp, op, btp, B, Sq, lens, off, bound, pages, page, pps, btrs, H, Hkv, Dh, qbs, qrs, kbs, krs, vbs, vrs,
                                      scale, cz, dt, ws.data_ptr(), wsb, st));
    else if (fp8)
      raise_on(awq_attn_kvcache_kv8(qp, kp, vp, ksp, vsp, op, B, Sq, lens, off, bound, L, H, Hkv, Dh, qbs, qrs, kbs, krs, vbs, vrs, ksbs, ksrs, vsbs,
                                    vsrs, scale, cz, dt, ws.data_ptr(), wsb, st));
    else
      raise_on(awq_attn_kvcache(qp, kp, vp, op, B, Sq, lens, off, bound, L, H, Hkv, Dh, qbs, qrs, kbs, krs, vbs, vrs, scale, cz, dt, ws.data_ptr(), wsb, st));
  }
  return out;
}

torch::Tensor attn_kvcache(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor seqlens_k,
                           int64_t max_seqlen_k, int64_t seqlen_offset, double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_kvcache", q, {k_cache, v_cache, nullptr, nullptr, nullptr}, seqlens_k, max_seqlen_k, seqlen_offset, softmax_scale,
                           causal);
}

torch::Tensor attn_kvcache_kv8(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor k_scale,
                               const torch::Tensor v_scale, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t seqlen_offset,
                               double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_kvcache_kv8", q, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, seqlens_k, max_seqlen_k, seqlen_offset,
                           softmax_scale, causal);
}

torch::Tensor attn_kvcache_paged(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor block_table,
                                 const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t seqlen_offset, double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_kvcache_paged", q, {k_pool, v_pool, nullptr, nullptr, &block_table}, seqlens_k, max_seqlen_k, seqlen_offset,
                           softmax_scale, causal);
}

torch::Tensor attn_kvcache_paged_kv8(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor k_scale,
                                     const torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor seqlens_k,
                                     int64_t max_seqlen_k, int64_t seqlen_offset, double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_kvcache_paged_kv8", q, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, seqlens_k, max_seqlen_k, seqlen_offset,
                           softmax_scale, causal);
}

// attn_kvcache_paged_shared[_kv8](q, pools .., block_table, seqlens_k, max_seqlen_k, group_members, group_prefix, seq_prefix, max_prefix,
// seqlen_offset, softmax_scale, causal) -> out: attn_kvcache_paged for a batch whose groups read their common prefix once (csrc/awq_shared.hpp).
static torch::Tensor attn_shared_impl(const char* who, const torch::Tensor& q, const KvTensors& kv, const torch::Tensor& seqlens_k,
                                      int64_t max_seqlen_k, const torch::Tensor& group_members, const torch::Tensor& group_prefix,
                                      const torch::Tensor& seq_prefix, int64_t max_prefix, int64_t seqlen_offset, double softmax_scale, bool causal) {
  const bool fp8 = kv.k_scale != nullptr;
  TORCH_CHECK(q.is_cuda(), who, ": q must live on the GPU");
  TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, who, ": float16 / bfloat16 only, got ", q.scalar_type());
  TORCH_CHECK(q.dim() == 4 && q.stride(3) == 1 && q.stride(2) == q.size(3), who, ": q [B, Sq, H, Dh] with contiguous heads is expected");
  const int64_t batch = q.size(0), sq = q.size(1), nheads = q.size(2), headdim = q.size(3);
  TORCH_CHECK(headdim == 64 || headdim == 128, who, ": head dim ", headdim, " is not supported (supported head dims: 64, 128)");
  check_kv(who, kv, q, "q", batch, /*contiguous=*/false);
  const torch::Tensor &k = kv.k, &v = kv.v, &bt = *kv.block_table;
  const int64_t pages = k.size(0), page = k.size(1), nheads_kv = k.size(2), cap = bt.size(1) * page;
  TORCH_CHECK(k.size(3) == headdim, who, ": k_pool / v_pool must be [num_pages, page_size, Hkv, ", headdim, "]");
  TORCH_CHECK(batch >= 1 && sq >= 1 && nheads_kv >= 1 && nheads % nheads_kv == 0, who,
              ": empty tensors are not supported and H must be a multiple of Hkv");
  TORCH_CHECK(max_seqlen_k >= 1 && max_seqlen_k <= cap, who, ": max_seqlen_k ", max_seqlen_k, " must lie in 1 .. ", cap, " (pages_per_seq * page_size)");
  TORCH_CHECK(seqlen_offset >= 0, who, ": seqlen_offset must not be negative");
  check_seqlens(who, "seqlens_k", seqlens_k, q, batch);
  check_seqlens(who, "seq_prefix", seq_prefix, q, batch);
  TORCH_CHECK(group_members.is_cuda() && group_members.device() == q.device() && group_members.scalar_type() == at::kInt && group_members.dim() == 2 &&
                  group_members.size(0) >= 1 && group_members.size(1) >= 1 && group_members.stride(1) == 1 &&
                  group_members.stride(0) >= group_members.size(1),
              who, ": group_members must be an int32 [num_groups, group_cap] tensor with a unit last stride on the GPU of q");
  const int64_t groups = group_members.size(0), gcap = group_members.size(1);
  TORCH_CHECK(group_prefix.is_cuda() && group_prefix.device() == q.device() && group_prefix.scalar_type() == at::kInt && group_prefix.dim() == 1 &&
                  group_prefix.size(0) == groups && group_prefix.is_contiguous(),
              who, ": group_prefix must be a contiguous int32 [num_groups] tensor on the GPU of q");
  TORCH_CHECK(gcap * sq * (nheads / nheads_kv) <= 128, who, ": group_cap * seqlen_q * (H / Hkv) = ", gcap * sq * (nheads / nheads_kv),
              " exceeds 128 (the rows of a group share one MFMA tile; list a wider group as several groups of the same prefix)");
  TORCH_CHECK(max_prefix >= 64 && max_prefix % 64 == 0 && max_prefix <= max_seqlen_k, who, ": max_prefix ", max_prefix,
              " must be a multiple of 64 in 64 .. max_seqlen_k = ", max_seqlen_k);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  at::Tensor out = torch::empty({batch, sq, nheads, headdim}, q.options().memory_format(at::MemoryFormat::Contiguous));
  const size_t wsb = awq_attn_kvcache_shared_workspace_bytes((int)batch, (int)nheads, (int)nheads_kv, (int)headdim, (int)sq, (int)max_prefix,
                                                             (int)max_seqlen_k);
  at::Tensor ws = torch::empty({(int64_t)wsb}, q.options().dtype(at::kByte));  // caching allocator: capturable
  void* st = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int B = (int)batch, Sq = (int)sq, H = (int)nheads, Hkv = (int)nheads_kv, Dh = (int)headdim;
  if (fp8)
    raise_on(awq_attn_kvcache_paged_shared_kv8(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), kv.k_scale->data_ptr<float>(), kv.v_scale->data_ptr<float>(), out.data_ptr(), bt.data_ptr<int>(), B,
        Sq, seqlens_k.data_ptr<int>(), (int)seqlen_offset, (int)max_seqlen_k, (int)pages, (int)page, (int)bt.size(1), bt.stride(0), H, Hkv, Dh,
        q.stride(0), q.stride(1), k.stride(0), k.stride(1), v.stride(0), v.stride(1), kv.k_scale->stride(0), kv.k_scale->stride(1),
        kv.v_scale->stride(0), kv.v_scale->stride(1), (float)softmax_scale, causal ? 1 : 0, dtype_code(q), group_members.data_ptr<int>(),
        group_prefix.data_ptr<int>(), seq_prefix.data_ptr<int>(), (int)groups, (int)gcap, group_members.stride(0), (int)max_prefix, ws.data_ptr(),
        wsb, st));
  else
    raise_on(awq_attn_kvcache_paged_shared(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), bt.data_ptr<int>(), B, Sq, seqlens_k.data_ptr<int>(), (int)seqlen_offset,
        (int)max_seqlen_k, (int)pages, (int)page, (int)bt.size(1), bt.stride(0), H, Hkv, Dh, q.stride(0), q.stride(1), k.stride(0), k.stride(1),
        v.stride(0), v.stride(1), (float)softmax_scale, causal ? 1 : 0, dtype_code(q), group_members.data_ptr<int>(), group_prefix.data_ptr<int>(),
        seq_prefix.data_ptr<int>(), (int)groups, (int)gcap, group_members.stride(0), (int)max_prefix, ws.data_ptr(), wsb, st));
  return out;
}

torch::Tensor attn_kvcache_paged_shared(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor block_table,
                                        const torch::Tensor seqlens_k, int64_t max_seqlen_k, const torch::Tensor group_members,
                                        const torch::Tensor group_prefix, const torch::Tensor seq_prefix, int64_t max_prefix, int64_t seqlen_offset,
                                        double softmax_scale, bool causal) {
  return attn_shared_impl("attn_kvcache_paged_shared", q, {k_pool, v_pool, nullptr, nullptr, &block_table}, seqlens_k, max_seqlen_k, group_members,
                          group_prefix, seq_prefix, max_prefix, seqlen_offset, softmax_scale, causal);
}

torch::Tensor attn_kvcache_paged_shared_kv8(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor k_scale,
                                            const torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor seqlens_k,
                                            int64_t max_seqlen_k, const torch::Tensor group_members, const torch::Tensor group_prefix,
                                            const torch::Tensor seq_prefix, int64_t max_prefix, int64_t seqlen_offset, double softmax_scale,
                                            bool causal) {
  return attn_shared_impl("attn_kvcache_paged_shared_kv8", q, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, seqlens_k, max_seqlen_k,
                          group_members, group_prefix, seq_prefix, max_prefix, seqlen_offset, softmax_scale, causal);
}

// kv_page_copy[_fp8](pools .., src_pages, dst_pages): page dst_pages[i] := page src_pages[i], one launch (the tail page of PageTable.fork)
static void kv_page_copy_impl(const char* who, torch::Tensor& k_pool, torch::Tensor& v_pool, torch::Tensor* k_scale, torch::Tensor* v_scale,
                              const torch::Tensor& src_pages, const torch::Tensor& dst_pages) {
  const bool fp8 = k_scale != nullptr;
  TORCH_CHECK(k_pool.is_cuda() && v_pool.is_cuda() && v_pool.device() == k_pool.device(), who, ": the pools must live on one GPU");
  TORCH_CHECK(k_pool.scalar_type() == v_pool.scalar_type() && k_pool.sizes() == v_pool.sizes() && k_pool.dim() == 4, who,
              ": k_pool and v_pool must have one shape [num_pages, page_size, Hkv, Dh] and one dtype");
  TORCH_CHECK(fp8 ? k_pool.element_size() == 1 : (k_pool.scalar_type() == at::kHalf || k_pool.scalar_type() == at::kBFloat16), who,
              ": float16 / bfloat16 pools, or one-byte FP8 codes with their scales, are expected");
  for (const torch::Tensor* t : {&k_pool, &v_pool})
    TORCH_CHECK(t->stride(3) == 1 && t->stride(2) == t->size(3), who, ": the pools must have contiguous heads");
  const int64_t pages = k_pool.size(0), page = k_pool.size(1), nheads_kv = k_pool.size(2), headdim = k_pool.size(3);
  TORCH_CHECK((headdim == 64 || headdim == 128) && page >= 64 && page % 64 == 0, who, ": head dim 64 / 128 and a page_size that is a multiple of 64");
  if (fp8)
    for (const torch::Tensor* t : {k_scale, v_scale})
      TORCH_CHECK(t->is_cuda() && t->device() == k_pool.device() && t->scalar_type() == at::kFloat && t->dim() == 3 && t->size(0) == pages &&
                      t->size(1) == page && t->size(2) == nheads_kv && t->stride(2) == 1,
                  who, ": the scale pools must be float32 [num_pages, page_size, Hkv] with a unit last stride on the GPU of the pools");
  for (const torch::Tensor* t : {&src_pages, &dst_pages})
    TORCH_CHECK(t->is_cuda() && t->device() == k_pool.device() && t->scalar_type() == at::kInt && t->dim() == 1 && t->size(0) == src_pages.size(0) &&
                    t->size(0) >= 1 && t->is_contiguous(),
                who, ": src_pages and dst_pages must be contiguous int32 [n >= 1] tensors on the GPU of the pools");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(k_pool.device());
  void* st = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  const int n = (int)src_pages.size(0);
  if (fp8)
    raise_on(awq_kv_page_copy_fp8(k_pool.data_ptr(), v_pool.data_ptr(), k_scale->data_ptr<float>(), v_scale->data_ptr<float>(),
                                  src_pages.data_ptr<int>(), dst_pages.data_ptr<int>(), n, (int)pages, (int)page, (int)nheads_kv, (int)headdim,
                                  k_pool.stride(0), k_pool.stride(1), v_pool.stride(0), v_pool.stride(1), k_scale->stride(0), k_scale->stride(1),
                                  v_scale->stride(0), v_scale->stride(1), st));
  else
    raise_on(awq_kv_page_copy(k_pool.data_ptr(), v_pool.data_ptr(), src_pages.data_ptr<int>(), dst_pages.data_ptr<int>(), n, (int)pages, (int)page,
                              (int)nheads_kv, (int)headdim, k_pool.stride(0), k_pool.stride(1), v_pool.stride(0), v_pool.stride(1), st));
}

void kv_page_copy(torch::Tensor k_pool, torch::Tensor v_pool, const torch::Tensor src_pages, const torch::Tensor dst_pages) {
  kv_page_copy_impl("kv_page_copy", k_pool, v_pool, nullptr, nullptr, src_pages, dst_pages);
}

void kv_page_copy_fp8(torch::Tensor k_pool, torch::Tensor v_pool, torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor src_pages,
                      const torch::Tensor dst_pages) {
  kv_page_copy_impl("kv_page_copy_fp8", k_pool, v_pool, &k_scale, &v_scale, src_pages, dst_pages);
}

// attn_prefill_kvcache[_kv8] / attn_prefill_paged[_kv8]: the arguments of their attn_kvcache* neighbours, served by the one-pass prefill
// kernel (csrc/awq_attn_prefill_cdna4.hip) for a prompt chunk of any length.
torch::Tensor attn_prefill_kvcache(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor seqlens_k,
                                   int64_t max_seqlen_k, int64_t seqlen_offset, double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_prefill_kvcache", q, {k_cache, v_cache, nullptr, nullptr, nullptr}, seqlens_k, max_seqlen_k, seqlen_offset,
                           softmax_scale, causal, true);
}

torch::Tensor attn_prefill_kvcache_kv8(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor k_scale,
                                       const torch::Tensor v_scale, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t seqlen_offset,
                                       double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_prefill_kvcache_kv8", q, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, seqlens_k, max_seqlen_k, seqlen_offset,
                           softmax_scale, causal, true);
}

torch::Tensor attn_prefill_paged(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor block_table,
                                 const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t seqlen_offset, double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_prefill_paged", q, {k_pool, v_pool, nullptr, nullptr, &block_table}, seqlens_k, max_seqlen_k, seqlen_offset,
                           softmax_scale, causal, true);
}

torch::Tensor attn_prefill_paged_kv8(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor k_scale,
                                     const torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor seqlens_k,
                                     int64_t max_seqlen_k, int64_t seqlen_offset, double softmax_scale, bool causal) {
  return attn_kvcache_impl("attn_prefill_paged_kv8", q, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, seqlens_k, max_seqlen_k, seqlen_offset,
                           softmax_scale, causal, true);
}

// rope_kv_store_natural_varq[_fp8] / rope_kv_store_paged_varq[_fp8](qkv [total_q, (H + 2 Hkv) Dh], freqs_table, caches or pools ..,
// cu_seqlens_q, max_seqlen_q, cache_seqlens, nheads, nheads_kv, q_out = None) -> q_out [total_q, H, Dh]
torch::Tensor rope_kv_store_natural_varq(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_cache, torch::Tensor v_cache,
                                         const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor cache_seqlens, int64_t nheads,
                                         int64_t nheads_kv, c10::optional<torch::Tensor> q_out) {
  return rope_store_impl("rope_kv_store_natural_varq", qkv, freqs_table, {k_cache, v_cache, nullptr, nullptr, nullptr}, &cache_seqlens, 0, nheads,
                         nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out});
}

torch::Tensor rope_kv_store_natural_varq_fp8(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_cache, torch::Tensor v_cache,
                                             torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q,
                                             const torch::Tensor cache_seqlens, int64_t nheads, int64_t nheads_kv,
                                             c10::optional<torch::Tensor> q_out) {
  return rope_store_impl("rope_kv_store_natural_varq_fp8", qkv, freqs_table, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, &cache_seqlens, 0,
                         nheads, nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out});
}

torch::Tensor rope_kv_store_paged_varq(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_pool, torch::Tensor v_pool,
                                       const torch::Tensor block_table, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q,
                                       const torch::Tensor cache_seqlens, int64_t nheads, int64_t nheads_kv, c10::optional<torch::Tensor> q_out) {
  return rope_store_impl("rope_kv_store_paged_varq", qkv, freqs_table, {k_pool, v_pool, nullptr, nullptr, &block_table}, &cache_seqlens, 0, nheads,
                         nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out});
}

torch::Tensor rope_kv_store_paged_varq_fp8(const torch::Tensor qkv, const torch::Tensor freqs_table, torch::Tensor k_pool, torch::Tensor v_pool,
                                           torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor block_table,
                                           const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor cache_seqlens,
                                           int64_t nheads, int64_t nheads_kv, c10::optional<torch::Tensor> q_out) {
  return rope_store_impl("rope_kv_store_paged_varq_fp8", qkv, freqs_table, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, &cache_seqlens, 0,
                         nheads, nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out});
}

// rope_kv_store_*_qknorm: each store binding with q_gamma, k_gamma (float32 [Dh]) and norm_eps behind its own arguments -- the per-head q/k
// RMSNorm of Qwen3 / Gemma-3 in front of the rotation, in the store launch (the C ABI's _qknorm siblings)
torch::Tensor rope_kv_store_natural_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache, int64_t start_pos,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_natural_qknorm", qkv, freqs, {k_cache, v_cache, nullptr, nullptr, nullptr}, nullptr, start_pos, nheads, nheads_kv, {}, &norm);
}

torch::Tensor rope_kv_store_natural_fp8_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor k_scale, torch::Tensor v_scale, int64_t start_pos,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_natural_fp8_qknorm", qkv, freqs, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, nullptr, start_pos, nheads, nheads_kv, {}, &norm);
}

torch::Tensor rope_kv_store_natural_pos_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_natural_pos_qknorm", qkv, freqs, {k_cache, v_cache, nullptr, nullptr, nullptr}, &cache_seqlens, 0, nheads, nheads_kv, {}, &norm);
}

torch::Tensor rope_kv_store_natural_pos_fp8_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_natural_pos_fp8_qknorm", qkv, freqs, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, &cache_seqlens, 0, nheads, nheads_kv, {}, &norm);
}

torch::Tensor rope_kv_store_paged_pos_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_pool, torch::Tensor v_pool, const torch::Tensor block_table, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_paged_pos_qknorm", qkv, freqs, {k_pool, v_pool, nullptr, nullptr, &block_table}, &cache_seqlens, 0, nheads, nheads_kv, {}, &norm);
}

torch::Tensor rope_kv_store_paged_pos_fp8_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_pool, torch::Tensor v_pool, torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_paged_pos_fp8_qknorm", qkv, freqs, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, &cache_seqlens, 0, nheads, nheads_kv, {}, &norm);
}

torch::Tensor rope_kv_store_natural_varq_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps, c10::optional<torch::Tensor> q_out) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_natural_varq_qknorm", qkv, freqs, {k_cache, v_cache, nullptr, nullptr, nullptr}, &cache_seqlens, 0, nheads, nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out}, &norm);
}

torch::Tensor rope_kv_store_natural_varq_fp8_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_cache, torch::Tensor v_cache, torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps, c10::optional<torch::Tensor> q_out) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_natural_varq_fp8_qknorm", qkv, freqs, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, &cache_seqlens, 0, nheads, nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out}, &norm);
}

torch::Tensor rope_kv_store_paged_varq_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_pool, torch::Tensor v_pool, const torch::Tensor block_table, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps, c10::optional<torch::Tensor> q_out) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_paged_varq_qknorm", qkv, freqs, {k_pool, v_pool, nullptr, nullptr, &block_table}, &cache_seqlens, 0, nheads, nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out}, &norm);
}

torch::Tensor rope_kv_store_paged_varq_fp8_qknorm(const torch::Tensor qkv, const torch::Tensor freqs, torch::Tensor k_pool, torch::Tensor v_pool, torch::Tensor k_scale, torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor cache_seqlens,
    int64_t nheads, int64_t nheads_kv, const torch::Tensor q_gamma, const torch::Tensor k_gamma, double norm_eps, c10::optional<torch::Tensor> q_out) {
  const QkNorm norm{&q_gamma, &k_gamma, norm_eps};
  return rope_store_impl("rope_kv_store_paged_varq_fp8_qknorm", qkv, freqs, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, &cache_seqlens, 0, nheads, nheads_kv, {&cu_seqlens_q, max_seqlen_q, &q_out}, &norm);
}

// attn_prefill_varq[_kv8] / attn_prefill_paged_varq[_kv8](q [total_q, H, Dh], caches or pools .., cu_seqlens_q, max_seqlen_q, seqlens_k,
// max_seqlen_k, lens_before_step, softmax_scale, causal, out = None) -> out [total_q, H, Dh]: the one-pass prefill kernel over packed queries
torch::Tensor attn_prefill_varq(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor cu_seqlens_q,
                                int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, bool lens_before_step,
                                double softmax_scale, bool causal, c10::optional<torch::Tensor> out) {
  return attn_kvcache_impl("attn_prefill_varq", q, {k_cache, v_cache, nullptr, nullptr, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale, causal, true,
                           {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step});
}

torch::Tensor attn_prefill_varq_kv8(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor k_scale,
                                    const torch::Tensor v_scale, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q,
                                    const torch::Tensor seqlens_k, int64_t max_seqlen_k, bool lens_before_step, double softmax_scale, bool causal,
                                    c10::optional<torch::Tensor> out) {
  return attn_kvcache_impl("attn_prefill_varq_kv8", q, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale, causal,
                           true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step});
}

torch::Tensor attn_prefill_paged_varq(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor block_table,
                                      const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k,
                                      bool lens_before_step, double softmax_scale, bool causal, c10::optional<torch::Tensor> out) {
  return attn_kvcache_impl("attn_prefill_paged_varq", q, {k_pool, v_pool, nullptr, nullptr, &block_table}, seqlens_k, max_seqlen_k, 0, softmax_scale,
                           causal, true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step});
}

torch::Tensor attn_prefill_paged_varq_kv8(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor k_scale,
                                          const torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor cu_seqlens_q,
                                          int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, bool lens_before_step,
                                          double softmax_scale, bool causal, c10::optional<torch::Tensor> out) {
  return attn_kvcache_impl("attn_prefill_paged_varq_kv8", q, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, seqlens_k, max_seqlen_k, 0,
                           softmax_scale, causal, true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step});
}

// attn_varq[_kv8] / attn_paged_varq[_kv8]: attn_prefill_varq[_kv8] / attn_prefill_paged_varq[_kv8] with (split_seqlen_q, split_min_keys) behind
// max_seqlen_k -- a mixed step: the packed split-KV pair serves the sequences with at most split_seqlen_q new tokens over at least
// split_min_keys keys, the one-pass kernel the others; three launches, the partials in a buffer of the caching allocator.
torch::Tensor attn_varq(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor cu_seqlens_q,
                        int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q, int64_t split_min_keys,
                        bool lens_before_step, double softmax_scale, bool causal, c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0, "attn_varq: split_seqlen_q must not be negative");
  return attn_kvcache_impl("attn_varq", q, {k_cache, v_cache, nullptr, nullptr, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale, causal, true,
                           {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys});
}

torch::Tensor attn_varq_kv8(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor k_scale,
                            const torch::Tensor v_scale, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor seqlens_k,
                            int64_t max_seqlen_k, int64_t split_seqlen_q, int64_t split_min_keys, bool lens_before_step, double softmax_scale,
                            bool causal, c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0, "attn_varq_kv8: split_seqlen_q must not be negative");
  return attn_kvcache_impl("attn_varq_kv8", q, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale, causal, true,
                           {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys});
}

torch::Tensor attn_paged_varq(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor block_table,
                              const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k,
                              int64_t split_seqlen_q, int64_t split_min_keys, bool lens_before_step, double softmax_scale, bool causal,
                              c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0, "attn_paged_varq: split_seqlen_q must not be negative");
  return attn_kvcache_impl("attn_paged_varq", q, {k_pool, v_pool, nullptr, nullptr, &block_table}, seqlens_k, max_seqlen_k, 0, softmax_scale, causal,
                           true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys});
}

torch::Tensor attn_paged_varq_kv8(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor k_scale,
                                  const torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor cu_seqlens_q,
                                  int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q,
                                  int64_t split_min_keys, bool lens_before_step, double softmax_scale, bool causal,
                                  c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0, "attn_paged_varq_kv8: split_seqlen_q must not be negative");
  return attn_kvcache_impl("attn_paged_varq_kv8", q, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, seqlens_k, max_seqlen_k, 0, softmax_scale,
                           causal, true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys});
}

// attn_varq_window[_kv8] / attn_paged_varq_window[_kv8]: attn_varq[_kv8] / attn_paged_varq[_kv8] with window_left behind split_min_keys -- row
// s of sequence b attends its own key and the window_left keys before it (flash-attn's window_size = (window_left, 0)); causal only.
torch::Tensor attn_varq_window(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor cu_seqlens_q,
                               int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q,
                               int64_t split_min_keys, int64_t window_left, bool lens_before_step, double softmax_scale, bool causal,
                               c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_varq_window: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_varq_window", q, {k_cache, v_cache, nullptr, nullptr, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale, causal,
                           true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left});
}

torch::Tensor attn_varq_window_kv8(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor k_scale,
                                   const torch::Tensor v_scale, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q,
                                   const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q, int64_t split_min_keys,
                                   int64_t window_left, bool lens_before_step, double softmax_scale, bool causal,
                                   c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_varq_window_kv8: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_varq_window_kv8", q, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale,
                           causal, true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left});
}

torch::Tensor attn_paged_varq_window(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor block_table,
                                     const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k,
                                     int64_t split_seqlen_q, int64_t split_min_keys, int64_t window_left, bool lens_before_step,
                                     double softmax_scale, bool causal, c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_paged_varq_window: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_paged_varq_window", q, {k_pool, v_pool, nullptr, nullptr, &block_table}, seqlens_k, max_seqlen_k, 0, softmax_scale,
                           causal, true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left});
}

torch::Tensor attn_paged_varq_window_kv8(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor k_scale,
                                         const torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor cu_seqlens_q,
                                         int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q,
                                         int64_t split_min_keys, int64_t window_left, bool lens_before_step, double softmax_scale, bool causal,
                                         c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_paged_varq_window_kv8: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_paged_varq_window_kv8", q, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, seqlens_k, max_seqlen_k, 0,
                           softmax_scale, causal, true,
                           {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left});
}

// attn_varq_softcap[_kv8] / attn_paged_varq_softcap[_kv8]: the four entries above with softcap behind window_left -- the logits become
// softcap * tanh(softmax_scale * q.k / softcap) in front of the causal / window mask (Gemma-2, Grok-1).  softcap = 0: the *_window entry.
torch::Tensor attn_varq_softcap(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor cu_seqlens_q,
                               int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q,
                               int64_t split_min_keys, int64_t window_left, double softcap, bool lens_before_step, double softmax_scale, bool causal,
                               c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_varq_softcap: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_varq_softcap", q, {k_cache, v_cache, nullptr, nullptr, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale, causal,
                           true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left, true, softcap});
}

torch::Tensor attn_varq_softcap_kv8(const torch::Tensor q, const torch::Tensor k_cache, const torch::Tensor v_cache, const torch::Tensor k_scale,
                                   const torch::Tensor v_scale, const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q,
                                   const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q, int64_t split_min_keys,
                                   int64_t window_left, double softcap, bool lens_before_step, double softmax_scale, bool causal,
                                   c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_varq_softcap_kv8: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_varq_softcap_kv8", q, {k_cache, v_cache, &k_scale, &v_scale, nullptr}, seqlens_k, max_seqlen_k, 0, softmax_scale,
                           causal, true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left, true, softcap});
}

torch::Tensor attn_paged_varq_softcap(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor block_table,
                                     const torch::Tensor cu_seqlens_q, int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k,
                                     int64_t split_seqlen_q, int64_t split_min_keys, int64_t window_left, double softcap, bool lens_before_step,
                                     double softmax_scale, bool causal, c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_paged_varq_softcap: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_paged_varq_softcap", q, {k_pool, v_pool, nullptr, nullptr, &block_table}, seqlens_k, max_seqlen_k, 0, softmax_scale,
                           causal, true, {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left, true, softcap});
}

torch::Tensor attn_paged_varq_softcap_kv8(const torch::Tensor q, const torch::Tensor k_pool, const torch::Tensor v_pool, const torch::Tensor k_scale,
                                         const torch::Tensor v_scale, const torch::Tensor block_table, const torch::Tensor cu_seqlens_q,
                                         int64_t max_seqlen_q, const torch::Tensor seqlens_k, int64_t max_seqlen_k, int64_t split_seqlen_q,
                                         int64_t split_min_keys, int64_t window_left, double softcap, bool lens_before_step, double softmax_scale, bool causal,
                                         c10::optional<torch::Tensor> out) {
  TORCH_CHECK(split_seqlen_q >= 0 && window_left >= 0, "attn_paged_varq_softcap_kv8: split_seqlen_q and window_left must not be negative");
  return attn_kvcache_impl("attn_paged_varq_softcap_kv8", q, {k_pool, v_pool, &k_scale, &v_scale, &block_table}, seqlens_k, max_seqlen_k, 0,
                           softmax_scale, causal, true,
                           {&cu_seqlens_q, max_seqlen_q, &out, lens_before_step, split_seqlen_q, split_min_keys, window_left, true, softcap});
}

// (splits, chunk) of awq_attn_varq_window_plan: attn_kvcache_plan's for min(max_seqlen_k, window_left + split_seqlen_q + 63).  Host only.
std::tuple<int64_t, int64_t> attn_varq_window_plan(int64_t batch, int64_t nheads, int64_t nheads_kv, int64_t head_dim, int64_t split_seqlen_q,
                                                   int64_t max_seqlen_k, int64_t window_left) {
  int splits = 1, chunk = 0;
  raise_on(awq_attn_varq_window_plan((int)batch, (int)nheads, (int)nheads_kv, (int)head_dim, (int)split_seqlen_q, (int)max_seqlen_k,
                                     (int)std::min<int64_t>(window_left, 0x7FFFFFFF), &splits, &chunk));
  return {splits, chunk};
}

// (splits, chunk) of awq_attn_varq_split_plan: attn_kvcache_plan's for the same bound.  Host only.
std::tuple<int64_t, int64_t> attn_varq_split_plan(int64_t batch, int64_t nheads, int64_t nheads_kv, int64_t head_dim, int64_t split_seqlen_q,
                                                  int64_t max_seqlen_k) {
  int splits = 1, chunk = 0;
  raise_on(awq_attn_varq_split_plan((int)batch, (int)nheads, (int)nheads_kv, (int)head_dim, (int)split_seqlen_q, (int)max_seqlen_k, &splits, &chunk));
  return {splits, chunk};
}

// (q_tile_rows, blocks) of awq_attn_varq_plan.  Host only.
std::tuple<int64_t, int64_t> attn_varq_plan(int64_t batch, int64_t nheads, int64_t nheads_kv, int64_t head_dim, int64_t max_seqlen_q) {
  int rows = 0, blocks = 0;
  raise_on(awq_attn_varq_plan((int)batch, (int)nheads, (int)nheads_kv, (int)head_dim, (int)max_seqlen_q, &rows, &blocks));
  return {rows, blocks};
}

// (splits, chunk) of awq_attn_kvcache_plan, made from the bound alone.  Host only.
std::tuple<int64_t, int64_t> attn_kvcache_plan(int64_t batch, int64_t nheads, int64_t nheads_kv, int64_t head_dim, int64_t seqlen_q,
                                               int64_t max_seqlen_k) {
  int splits = 1, chunk = 0;
  raise_on(awq_attn_kvcache_plan((int)batch, (int)nheads, (int)nheads_kv, (int)head_dim, (int)seqlen_q, (int)max_seqlen_k, &splits, &chunk));
  return {splits, chunk};
}

// the checks attn_prefill_kv8 and attn_splitkv_kv8 share: q [B, Sq, H, Dh] of T, k / v codes [B, Sk, Hkv, Dh], k_scale / v_scale [B, Sk, Hkv]
static void check_kv8_attn(const char* who, const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v, const torch::Tensor& k_scale,
                           const torch::Tensor& v_scale, bool causal) {
  TORCH_CHECK(q.scalar_type() != at::kFloat, who, ": float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(q.is_cuda(), who, ": q must live on the GPU");
  TORCH_CHECK(q.scalar_type() == at::kHalf || q.scalar_type() == at::kBFloat16, who, ": float16 / bfloat16 only, got ", q.scalar_type());
  const char* cname[2] = {"k", "v"};
  const char* sname[2] = {"k_scale", "v_scale"};
  const torch::Tensor* codes[2] = {&k, &v};
  const torch::Tensor* scales[2] = {&k_scale, &v_scale};
  TORCH_CHECK(q.dim() == 4, who, ": q must be [B, Sq, H, Dh]");
  const int64_t batch = q.size(0), sq = q.size(1), nheads = q.size(2), headdim = q.size(3);
  TORCH_CHECK(headdim == 64 || headdim == 128, who, ": head dim ", headdim, " is not supported (supported head dims: 64, 128)");
  TORCH_CHECK(q.stride(3) == 1 && q.stride(2) == headdim, who, ": the heads of q must be contiguous (stride(3) == 1, stride(2) == Dh)");
  for (int i = 0; i < 2; ++i) {
    TORCH_CHECK(codes[i]->is_cuda() && codes[i]->device() == q.device(), who, ": ", cname[i], " must live on the GPU of q");
    TORCH_CHECK(is_kv8_code(*codes[i]), who, ": ", cname[i], " must be float8_e4m3fn or uint8, got ", codes[i]->scalar_type());
    TORCH_CHECK(codes[i]->dim() == 4 && codes[i]->size(0) == batch && codes[i]->size(3) == headdim, who, ": ", cname[i], " must be [B, Sk, Hkv, ",
                headdim, "]");
    TORCH_CHECK(codes[i]->stride(3) == 1 && codes[i]->stride(2) == headdim, who, ": the heads of ", cname[i],
                " must be contiguous (stride(3) == 1, stride(2) == Dh)");
    TORCH_CHECK(scales[i]->is_cuda() && scales[i]->device() == q.device(), who, ": ", sname[i], " must live on the GPU of q");
    TORCH_CHECK(scales[i]->scalar_type() == at::kFloat, who, ": ", sname[i], " must be float32, got ", scales[i]->scalar_type());
    TORCH_CHECK(scales[i]->dim() == 3 && scales[i]->size(0) == batch && scales[i]->size(1) == codes[i]->size(1) &&
                    scales[i]->size(2) == codes[i]->size(2) && scales[i]->stride(2) == 1,
                who, ": ", sname[i], " must be [B, Sk, Hkv] of ", cname[i], " with a unit last stride");
  }
  TORCH_CHECK(v.sizes() == k.sizes(), who, ": k and v must have one shape [B, Sk, Hkv, Dh]");
  const int64_t sk = k.size(1), nheads_kv = k.size(2);
  TORCH_CHECK(batch >= 1 && sq >= 1 && sk >= 1 && nheads_kv >= 1 && nheads % nheads_kv == 0, who,
              ": empty tensors are not supported and H must be a multiple of Hkv");
  TORCH_CHECK(!causal || sq <= sk, who, ": causal attention needs seqlen_q <= seqlen_k, got ", sq, " > ", sk);
}

// attn_splitkv_kv8(q, k, v, k_scale, v_scale, softmax_scale, causal) -> out: attn_splitkv on the FP8 cache; attn_prefill_kv8 where the plan
// does not split.  Bit-identical to attn_splitkv / attn_prefill on the dequantised tensors.  The workspace is the caching allocator's: capturable.
static torch::Tensor attn_kv8_impl(const char* who, bool split, const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
                                   const torch::Tensor& k_scale, const torch::Tensor& v_scale, double softmax_scale, bool causal) {
  check_kv8_attn(who, q, k, v, k_scale, v_scale, causal);
  const int64_t batch = q.size(0), sq = q.size(1), nheads = q.size(2), headdim = q.size(3), sk = k.size(1), nheads_kv = k.size(2);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(q.device());
  at::Tensor out = torch::empty({batch, sq, nheads, headdim}, q.options().memory_format(at::MemoryFormat::Contiguous));
  void* st = (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream();
  if (!split) {
    raise_on(awq_attn_prefill_kv8(q.data_ptr(), k.data_ptr(), v.data_ptr(), k_scale.data_ptr<float>(), v_scale.data_ptr<float>(), out.data_ptr(),
                                  (int)batch, (int)sq, (int)sk, (int)nheads, (int)nheads_kv, (int)headdim, q.stride(0), q.stride(1), k.stride(0),
                                  k.stride(1), v.stride(0), v.stride(1), k_scale.stride(0), k_scale.stride(1), v_scale.stride(0),
                                  v_scale.stride(1), (float)softmax_scale, causal ? 1 : 0, dtype_code(q), st));
    return out;
  }
  const size_t wsb = awq_attn_splitkv_workspace_bytes((int)batch, (int)nheads, (int)nheads_kv, (int)headdim, (int)sq, (int)sk, causal ? 1 : 0);
  at::Tensor ws;
  if (wsb) ws = torch::empty({(int64_t)wsb}, q.options().dtype(at::kByte));  // caching allocator: capturable
  raise_on(awq_attn_splitkv_kv8(q.data_ptr(), k.data_ptr(), v.data_ptr(), k_scale.data_ptr<float>(), v_scale.data_ptr<float>(), out.data_ptr(),
                                (int)batch, (int)sq, (int)sk, (int)nheads, (int)nheads_kv, (int)headdim, q.stride(0), q.stride(1), k.stride(0),
                                k.stride(1), v.stride(0), v.stride(1), k_scale.stride(0), k_scale.stride(1), v_scale.stride(0), v_scale.stride(1),
                                (float)softmax_scale, causal ? 1 : 0, dtype_code(q), wsb ? ws.data_ptr() : nullptr, wsb, st));
  return out;
}

torch::Tensor attn_prefill_kv8(const torch::Tensor q, const torch::Tensor k, const torch::Tensor v, const torch::Tensor k_scale,
                               const torch::Tensor v_scale, double softmax_scale, bool causal) {
  return attn_kv8_impl("attn_prefill_kv8", false, q, k, v, k_scale, v_scale, softmax_scale, causal);
}

torch::Tensor attn_splitkv_kv8(const torch::Tensor q, const torch::Tensor k, const torch::Tensor v, const torch::Tensor k_scale,
                               const torch::Tensor v_scale, double softmax_scale, bool causal) {
  return attn_kv8_impl("attn_splitkv_kv8", true, q, k, v, k_scale, v_scale, softmax_scale, causal);
}

// flash_attn_varlen_qkvpacked_func's forward (tinychat/models/internvl/internvit.py:45-90) on the gfx950 tower kernel
// (csrc/awq_attn_tower_cdna4.hip): qkv [nnz, 3, H, Dh] with contiguous heads, cu_seqlens int32 [nseq + 1] on the same GPU, read by the
// kernel only (no host copy, no sync).  Returns [nnz, H, Dh] contiguous; rows >= cu_seqlens[-1] are left unwritten.
torch::Tensor attn_varlen_qkvpacked(const torch::Tensor qkv, const torch::Tensor cu_seqlens, int64_t max_seqlen, double softmax_scale,
                                    bool causal) {
  TORCH_CHECK(qkv.scalar_type() != at::kFloat, "attn_varlen_qkvpacked: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(qkv.is_cuda() && cu_seqlens.is_cuda() && cu_seqlens.device() == qkv.device(),
              "attn_varlen_qkvpacked: qkv and cu_seqlens must live on the same GPU");
  TORCH_CHECK(qkv.scalar_type() == at::kHalf || qkv.scalar_type() == at::kBFloat16, "attn_varlen_qkvpacked: float16 / bfloat16 only, got ",
              qkv.scalar_type());
  TORCH_CHECK(!causal, "attn_varlen_qkvpacked: causal attention is not supported (encoder towers only)");
  TORCH_CHECK(qkv.dim() == 4 && qkv.size(1) == 3, "attn_varlen_qkvpacked: qkv [nnz, 3, H, Dh]");
  const int64_t nnz = qkv.size(0), nheads = qkv.size(2), headdim = qkv.size(3);
  TORCH_CHECK(headdim == 64 || headdim == 72, "attn_varlen_qkvpacked: head dim ", headdim, " is not supported (supported head dims: 64, 72)");
  TORCH_CHECK(cu_seqlens.scalar_type() == at::kInt && cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2 && cu_seqlens.is_contiguous(),
              "attn_varlen_qkvpacked: cu_seqlens must be a contiguous int32 tensor of nseq + 1 entries");
  TORCH_CHECK(nnz >= 1 && nheads >= 1 && max_seqlen >= 1 && max_seqlen <= 0x7FFFFFFF, "attn_varlen_qkvpacked: empty tensors are not supported");
  TORCH_CHECK(qkv.stride(3) == 1 && qkv.stride(2) == headdim && qkv.stride(1) == nheads * headdim,
              "attn_varlen_qkvpacked: the heads of qkv must be contiguous (stride(3) == 1, stride(2) == Dh, stride(1) == H * Dh)");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(qkv.device());
  at::Tensor out = torch::empty({nnz, nheads, headdim}, qkv.options().memory_format(at::MemoryFormat::Contiguous));
  const char* base = (const char*)qkv.data_ptr();
  const int64_t step = qkv.stride(1) * (int64_t)qkv.element_size();
  raise_on(awq_attn_varlen(base, base + step, base + 2 * step, out.data_ptr(), (const int*)cu_seqlens.data_ptr(), (int)(cu_seqlens.numel() - 1),
                           (int)max_seqlen, nnz, (int)nheads, (int)headdim, qkv.stride(0), qkv.stride(0), qkv.stride(0), (float)softmax_scale,
                           0, dtype_code(qkv), (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// fused_rope_with_pos_forward_func(input, freqs, transpose_output_memory) (rope_new/fused_rope_with_pos.cu:263-333): input [n0, n1, h, d]
// with any strides, freqs fp32 with last dim d2, read at (i1 * n0 + i0) * d2 + c -- the reference's own index.  The result has input's
// shape; with transpose_output_memory its memory is that of a contiguous [n1, n0, h, d] tensor (:303-307).
torch::Tensor fused_rope_with_pos_forward_func(const torch::Tensor& input, const torch::Tensor& freqs, const bool transpose_output_memory) {
  TORCH_CHECK(input.scalar_type() != at::kFloat,
              "fused_rope_with_pos_forward_func: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  TORCH_CHECK(input.is_cuda() && freqs.is_cuda() && freqs.device() == input.device(), "fused_rope_with_pos_forward_func: tensors must live on the same GPU");
  TORCH_CHECK(input.scalar_type() == at::kHalf || input.scalar_type() == at::kBFloat16,
              "fused_rope_with_pos_forward_func: float16 / bfloat16 only, got ", input.scalar_type());
  TORCH_CHECK(freqs.scalar_type() == at::kFloat, "fused_rope_with_pos_forward_func: freqs must be float32");
  TORCH_CHECK(input.dim() == 4 && freqs.dim() >= 1, "fused_rope_with_pos_forward_func: input must be 4-D");
  const int64_t n0 = input.size(0), n1 = input.size(1), h = input.size(2), d = input.size(3), d2 = freqs.size(-1);
  TORCH_CHECK(n0 >= 1 && n1 >= 1 && h >= 1 && d2 <= d && freqs.numel() >= n0 * n1 * d2,
              "fused_rope_with_pos_forward_func: freqs must hold n0 * n1 * d2 angles with d2 <= head dim");
  TORCH_CHECK(d % 8 == 0 && d2 % 16 == 0 && d2 >= 16, "fused_rope_with_pos_forward_func: head dim % 8 == 0 and rotary dim % 16 == 0 are required");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
  // the kernel reads 16 bytes at a time: a view whose last stride is not 1, or whose strides / base are not 16-byte multiples, is copied once
  at::Tensor x = input;
  if (x.stride(3) != 1 || x.stride(0) % 8 || x.stride(1) % 8 || x.stride(2) % 8 || (reinterpret_cast<uintptr_t>(x.data_ptr()) & 15)) x = input.contiguous();
  at::Tensor fr = freqs.is_contiguous() && (reinterpret_cast<uintptr_t>(freqs.data_ptr()) & 15) == 0 ? freqs : freqs.contiguous().clone();
  auto opt = input.options().requires_grad(false);
  at::Tensor out = transpose_output_memory ? torch::empty({n1, n0, h, d}, opt).transpose(0, 1) : torch::empty({n0, n1, h, d}, opt);
  raise_on(awq_rope_with_pos(x.data_ptr(), fr.data_ptr<float>(), out.data_ptr(), (int)n0, (int)n1, (int)h, (int)d, (int)d2, x.stride(0), x.stride(1),
                             x.stride(2), out.stride(0), out.stride(1), out.stride(2), dtype_code(x),
                             (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// rotary_embedding_neox(positions, query, key, head_size, cos_sin_cache) (position_embedding/pos_encoding_kernels.cu:55-87): in place on
// contiguous query and key [.., num_heads, head_size] (the same head count, as the reference assumes), positions int64, cache [max_pos, rot_dim].
void rotary_embedding_neox(torch::Tensor& positions, torch::Tensor& query, torch::Tensor& key, int head_size, torch::Tensor& cos_sin_cache) {
  TORCH_CHECK(query.scalar_type() != at::kFloat, "rotary_embedding_neox: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  for (const torch::Tensor* t : std::initializer_list<const torch::Tensor*>{&positions, &query, &key, &cos_sin_cache})
    TORCH_CHECK(t->is_cuda() && t->device() == query.device() && t->is_contiguous(), "rotary_embedding_neox: contiguous tensors on one GPU are expected");
  TORCH_CHECK((query.scalar_type() == at::kHalf || query.scalar_type() == at::kBFloat16) && key.scalar_type() == query.scalar_type() &&
                  cos_sin_cache.scalar_type() == query.scalar_type() && positions.scalar_type() == at::kLong,
              "rotary_embedding_neox: float16 / bfloat16 query, key and cache of one dtype and int64 positions are expected");
  TORCH_CHECK(query.dim() >= 2 && cos_sin_cache.dim() == 2 && query.size(-1) == head_size && key.sizes() == query.sizes(),
              "rotary_embedding_neox: query and key [.., num_heads, head_size] of one shape, cache [max_position, rot_dim]");
  const int64_t heads = query.size(-2), rot = cos_sin_cache.size(1);
  if (query.numel() == 0) return;
  const int64_t tokens = query.numel() / (heads * head_size);
  TORCH_CHECK(positions.numel() == tokens, "rotary_embedding_neox: one position per token is expected");
  TORCH_CHECK(rot % 16 == 0 && rot >= 16 && rot <= head_size && head_size % 8 == 0, "rotary_embedding_neox: rot_dim % 16 == 0 and rot_dim <= head_size are required");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(query.device());
  raise_on(awq_rope_neox_inplace((const long long*)positions.data_ptr<int64_t>(), query.data_ptr(), key.data_ptr(), cos_sin_cache.data_ptr(), (int)tokens,
                                 (int)heads, head_size, (int)rot, (int)cos_sin_cache.size(0), dtype_code(query),
                                 (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
}

torch::Tensor rmsnorm_forward_cdna4(torch::Tensor in_feats, torch::Tensor gamma, double eps, torch::Tensor kernel, torch::Tensor sz_packed,
                                    c10::optional<torch::Tensor> bias, bool fused_gate_up) {
  TORCH_CHECK(in_feats.is_cuda() && gamma.is_cuda() && kernel.is_cuda() && sz_packed.is_cuda());
  TORCH_CHECK(in_feats.is_contiguous() && gamma.is_contiguous() && kernel.is_contiguous() && sz_packed.is_contiguous());
  TORCH_CHECK((in_feats.scalar_type() == at::kBFloat16 || in_feats.scalar_type() == at::kHalf) && gamma.scalar_type() == in_feats.scalar_type() &&
              kernel.scalar_type() == at::kShort && sz_packed.scalar_type() == at::kInt);
  const int64_t n = kernel.size(0) * 4, k = in_feats.size(-1);
  TORCH_CHECK(k > 0 && in_feats.numel() % k == 0 && kernel.numel() == n / 4 * k && gamma.numel() == k);
  TORCH_CHECK(sz_packed.numel() == n * (k / 128), "sz_packed must be int32 [n/16, k/128, 16]");
  const int64_t m = in_feats.numel() / k;
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = fused_gate_up ? n / 2 : n;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  const void* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() && bias->scalar_type() == in_feats.scalar_type() && bias->numel() == n);
    bp = bias->data_ptr();
  }
  raise_on(awq_w4a16_rmsnorm_forward_cdna4(in_feats.data_ptr(), gamma.data_ptr(), (float)eps, kernel.data_ptr(), sz_packed.data_ptr(), bp,
                                           out.data_ptr(), (int)m, (int)n, (int)k, 128, dtype_code(in_feats), fused_gate_up ? 1 : 0,
                                           (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}


// QuantLlamaMLP.our_llama_mlp for any row count on the 8 + 8 interleaved gate / up pair: out [.., n2 / 2]
torch::Tensor mlp_gate_up_forward_cdna4(torch::Tensor in_feats, torch::Tensor kernel, torch::Tensor sz_packed, c10::optional<torch::Tensor> sz_half) {
  TORCH_CHECK(in_feats.is_cuda() && kernel.is_cuda() && sz_packed.is_cuda());
  TORCH_CHECK(in_feats.is_contiguous() && kernel.is_contiguous() && sz_packed.is_contiguous());
  TORCH_CHECK((in_feats.scalar_type() == at::kBFloat16 || in_feats.scalar_type() == at::kHalf) && kernel.scalar_type() == at::kShort &&
              sz_packed.scalar_type() == at::kInt);
  const int64_t n2 = kernel.size(0) * 4, k = in_feats.size(-1);
  TORCH_CHECK(k > 0 && in_feats.numel() % k == 0 && kernel.numel() == n2 / 4 * k);
  TORCH_CHECK(sz_packed.numel() == n2 * (k / 128), "sz_packed must be int32 [n2/16, k/128, 16]");
  const void* hp = nullptr;
  if (sz_half.has_value() && sz_half->defined()) {
    TORCH_CHECK(sz_half->is_cuda() && sz_half->is_contiguous() && sz_half->scalar_type() == at::kInt && sz_half->numel() == sz_packed.numel());
    hp = sz_half->data_ptr();
  }
  const int64_t m = in_feats.numel() / k;
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = n2 / 2;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  if (m == 0) return out;
  // optional scratch of the prefill plan (block pairs for the columns behind the full rounds): torch's caching allocator, stream-ordered, capture-safe
  at::Tensor ws;
  void* wsp = nullptr;
  const size_t wsb = awq_w4a16_mlp_gate_up_forward_cdna4_workspace_bytes((int)m, (int)n2, (int)k);
  if (wsb) {
    ws = torch::empty({(int64_t)wsb}, in_feats.options().dtype(at::kByte));
    wsp = ws.data_ptr();
  }
  raise_on(awq_w4a16_mlp_gate_up_forward_cdna4_ws(in_feats.data_ptr(), kernel.data_ptr(), sz_packed.data_ptr(), hp, out.data_ptr(), (int)m, (int)n2,
                                                  (int)k, 128, dtype_code(in_feats), wsp, wsb,
                                                  (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// "sz_half" side buffer of the decode kernels; returns (int32 [n/16, k/128, 16], exact).  Synchronises once (reads the flag).
std::tuple<torch::Tensor, bool> pack_szh_cdna4(torch::Tensor scales, torch::Tensor zeros, int k) {
  TORCH_CHECK(scales.is_cuda() && zeros.is_cuda() && scales.is_contiguous() && zeros.is_contiguous());
  TORCH_CHECK(scales.scalar_type() == zeros.scalar_type() && scales.sizes() == zeros.sizes() && scales.dim() == 2);
  TORCH_CHECK(scales.scalar_type() == at::kBFloat16 || scales.scalar_type() == at::kHalf);
  const int64_t n = scales.size(1);
  TORCH_CHECK(n % 16 == 0 && k % 128 == 0 && scales.size(0) * 128 >= k);
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(scales.device());
  at::Tensor out = torch::empty({n / 16, k / 128, 16}, scales.options().dtype(at::kInt));
  at::Tensor flag = torch::zeros({1}, scales.options().dtype(at::kInt));
  raise_on(awq_pack_szh_cdna4(scales.data_ptr(), zeros.data_ptr(), out.data_ptr(), (int*)flag.data_ptr(), (int)n, k, dtype_code(scales),
                              (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return {out, flag.item<int>() == 0};
}

// decode (<= 8 rows) on cdna4 weights + sz_half; epilogue 0: x.W^T (+bias), 1: stacked [gate; up] -> silu(gate)*up, 2: interleaved 8 + 8
torch::Tensor decode_cdna4(torch::Tensor in_feats, torch::Tensor kernel, torch::Tensor sz_half, c10::optional<torch::Tensor> bias,
                           int epilogue) {
  TORCH_CHECK(in_feats.is_cuda() && kernel.is_cuda() && sz_half.is_cuda());
  TORCH_CHECK(in_feats.is_contiguous() && kernel.is_contiguous() && sz_half.is_contiguous());
  TORCH_CHECK((in_feats.scalar_type() == at::kBFloat16 || in_feats.scalar_type() == at::kHalf) && kernel.scalar_type() == at::kShort &&
              sz_half.scalar_type() == at::kInt);
  const int64_t n = kernel.size(0) * 4, k = in_feats.size(-1);
  TORCH_CHECK(k > 0 && in_feats.numel() % k == 0 && kernel.numel() == n / 4 * k);
  TORCH_CHECK(sz_half.numel() == n * (k / 128), "sz_half must be int32 [n/16, k/128, 16]");
  const int64_t m = in_feats.numel() / k;
  std::vector<int64_t> shape = in_feats.sizes().vec();
  shape.back() = epilogue ? n / 2 : n;
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  at::Tensor out = torch::empty(shape, in_feats.options());
  const void* bp = nullptr;
  if (bias.has_value() && bias->defined()) {
    TORCH_CHECK(bias->is_cuda() && bias->is_contiguous() && bias->scalar_type() == in_feats.scalar_type() && bias->numel() == n);
    bp = bias->data_ptr();
  }
  raise_on(awq_w4a16_decode_cdna4(in_feats.data_ptr(), kernel.data_ptr(), sz_half.data_ptr(), bp, out.data_ptr(), (int)m, (int)n, (int)k,
                                  128, dtype_code(in_feats), epilogue, (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
  return out;
}

// ---------------------------------------------------------------------------------------------------------------
// W8A8 family (awq/kernels/csrc/w8a8/; pybind.cpp:30-37).  Outputs are written into the caller's buffers, nothing is returned.  The
// reference checks nothing and launches on the default stream of the current device; here every tensor is checked and the launch goes
// to the current stream of the tensors' device.
// ---------------------------------------------------------------------------------------------------------------
void w8a8_check(const char* fn, std::initializer_list<const torch::Tensor*> ts) {
  const torch::Tensor& first = **ts.begin();
  for (const torch::Tensor* t : ts)
    TORCH_CHECK(t->is_cuda() && t->device() == first.device() && t->is_contiguous(), fn, ": contiguous tensors on one GPU are expected");
}

void w8a8_gemm_common(const char* fn, torch::Tensor& in_feats, torch::Tensor& kernel, torch::Tensor& wscales, torch::Tensor& ascales,
                      torch::Tensor& out_feats, const torch::Tensor* bias) {
  TORCH_CHECK(out_feats.scalar_type() != at::kFloat && wscales.scalar_type() != at::kFloat && ascales.scalar_type() != at::kFloat,
              fn, ": float32 is not supported by the MI355X build (scales, bias and output are float16)");
  w8a8_check(fn, {&in_feats, &kernel, &wscales, &ascales, &out_feats});
  if (bias) w8a8_check(fn, {&in_feats, bias});
  TORCH_CHECK(in_feats.scalar_type() == at::kChar && kernel.scalar_type() == at::kChar, fn, ": int8 in_feats [M, K] and kernel [N, K] are expected");
  TORCH_CHECK(out_feats.scalar_type() == at::kHalf && wscales.scalar_type() == at::kHalf && ascales.scalar_type() == at::kHalf &&
                  (!bias || bias->scalar_type() == at::kHalf),
              fn, ": float16 wscales, ascales, bias and out_feats are expected");
  TORCH_CHECK(in_feats.dim() == 2 && kernel.dim() == 2 && out_feats.dim() >= 2, fn, ": in_feats [M, K], kernel [N, K], out_feats [.., M, N] are expected");
  const int64_t m = in_feats.size(0), k = in_feats.size(1), n = kernel.size(0);
  TORCH_CHECK(kernel.size(1) == k && out_feats.size(-2) == m && out_feats.size(-1) == n && out_feats.numel() == m * n && wscales.numel() == n &&
                  ascales.numel() >= m && (!bias || bias->numel() == n),
              fn, ": shapes do not match (in_feats [M, K], kernel [N, K], wscales [N], ascales [M], bias [N], out_feats [M, N])");
  TORCH_CHECK(m >= 1 && k % 16 == 0 && n % 8 == 0 && m <= INT32_MAX && n <= INT32_MAX && k <= INT32_MAX, fn, ": K % 16 == 0 and N % 8 == 0 are required");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(in_feats.device());
  raise_on(awq_w8a8_gemm(in_feats.data_ptr(), kernel.data_ptr(), wscales.data_ptr(), ascales.data_ptr(), bias ? bias->data_ptr() : nullptr,
                         out_feats.data_ptr(), (int)m, (int)n, (int)k, (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
}

// w8a8_gemm_forward_cuda(in_feats, kernel, wscales, ascales, out_feats) (w8a8_gemm_cuda.cu:907-953)
void w8a8_gemm_forward_cuda(torch::Tensor _in_feats, torch::Tensor _kernel, torch::Tensor _wscales, torch::Tensor _ascales, torch::Tensor _out_feats) {
  w8a8_gemm_common("w8a8_gemm_forward_cuda", _in_feats, _kernel, _wscales, _ascales, _out_feats, nullptr);
}
// w8a8_gemm_fuse_bias_forward_cuda(in_feats, kernel, wscales, ascales, out_feats, bias) (w8a8_gemm_cuda.cu:586-633)
void w8a8_gemm_fuse_bias_forward_cuda(torch::Tensor _in_feats, torch::Tensor _kernel, torch::Tensor _wscales, torch::Tensor _ascales,
                                      torch::Tensor _out_feats, torch::Tensor _bias) {
  w8a8_gemm_common("w8a8_gemm_fuse_bias_forward_cuda", _in_feats, _kernel, _wscales, _ascales, _out_feats, &_bias);
}

// invoke_quant(out, input, scale) (quantization.cu:97-112): input T [.., hidden], out int8 of the same shape, scale fp16 [tokens]
void invoke_quant(torch::Tensor& out, torch::Tensor& input, torch::Tensor& scale) {
  TORCH_CHECK(input.scalar_type() != at::kFloat, "invoke_quant: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  w8a8_check("invoke_quant", {&input, &out, &scale});
  TORCH_CHECK((input.scalar_type() == at::kHalf || input.scalar_type() == at::kBFloat16) && out.scalar_type() == at::kChar &&
                  scale.scalar_type() == at::kHalf,
              "invoke_quant: float16 / bfloat16 input, int8 out and float16 scale are expected");
  TORCH_CHECK(input.dim() >= 1 && input.numel() > 0, "invoke_quant: input [.., hidden] is expected");
  const int64_t k = input.size(-1), m = input.numel() / k;
  TORCH_CHECK(out.numel() == input.numel() && scale.numel() >= m && k % 8 == 0 && m <= INT32_MAX && k <= INT32_MAX,
              "invoke_quant: out of input's size, one scale per token and hidden % 8 == 0 are required");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
  raise_on(awq_quant_per_token(input.data_ptr(), out.data_ptr(), scale.data_ptr(), (int)m, (int)k, dtype_code(input),
                               (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
}

// gelu_and_quant(out, input, scale_out, tmp) (act.cu:82-95): fp16 input [.., d]; tmp receives the fp16 GELU, out / scale_out its quantisation
void gelu_and_quant(torch::Tensor& out, torch::Tensor& input, torch::Tensor& scale_out, torch::Tensor& tmp) {
  TORCH_CHECK(input.scalar_type() != at::kFloat, "gelu_and_quant: float32 is not supported by the MI355X build (use float16)");
  w8a8_check("gelu_and_quant", {&input, &out, &scale_out, &tmp});
  TORCH_CHECK(input.scalar_type() == at::kHalf && tmp.scalar_type() == at::kHalf && scale_out.scalar_type() == at::kHalf &&
                  out.scalar_type() == at::kChar,
              "gelu_and_quant: float16 input, tmp and scale_out and int8 out are expected");
  TORCH_CHECK(input.dim() >= 1 && input.numel() > 0, "gelu_and_quant: input [.., d] is expected");
  const int64_t k = input.size(-1), m = input.numel() / k;
  TORCH_CHECK(out.numel() == input.numel() && tmp.numel() >= input.numel() && scale_out.numel() >= m && k % 8 == 0 && m <= INT32_MAX && k <= INT32_MAX,
              "gelu_and_quant: out and tmp of input's size, one scale per token and d % 8 == 0 are required");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
  raise_on(awq_gelu_quant_per_token(input.data_ptr(), out.data_ptr(), scale_out.data_ptr(), tmp.data_ptr(), (int)m, (int)k,
                                    (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
}

// rms_norm_general(out, input, weight, bias, scaling, epsilon, use_per_token_quant = true) (layernorm.cu:193-232): a LayerNorm with mean
// subtraction.  Per token: scaling fp16 [tokens] is written.  Per tensor: scaling[0] is read and multiplied, bias is ignored (:224-229).
void rms_norm_general(torch::Tensor& out, torch::Tensor& input, torch::Tensor& weight, c10::optional<torch::Tensor> bias, torch::Tensor& scaling,
                      double epsilon, bool use_per_token_quant) {
  TORCH_CHECK(input.scalar_type() != at::kFloat, "rms_norm_general: float32 is not supported by the MI355X build (use float16 or bfloat16)");
  w8a8_check("rms_norm_general", {&input, &out, &weight, &scaling});
  const bool has_bias = bias.has_value() && bias->defined();
  if (has_bias) w8a8_check("rms_norm_general", {&input, &*bias});
  TORCH_CHECK((input.scalar_type() == at::kHalf || input.scalar_type() == at::kBFloat16) && weight.scalar_type() == input.scalar_type() &&
                  (!has_bias || bias->scalar_type() == input.scalar_type()) && out.scalar_type() == at::kChar && scaling.scalar_type() == at::kHalf,
              "rms_norm_general: float16 / bfloat16 input, weight and bias of one dtype, int8 out and float16 scaling are expected");
  TORCH_CHECK(input.dim() >= 1 && input.numel() > 0, "rms_norm_general: input [.., hidden] is expected");
  const int64_t k = input.size(-1), m = input.numel() / k;
  TORCH_CHECK(out.numel() == input.numel() && weight.numel() == k && (!has_bias || bias->numel() == k) &&
                  scaling.numel() >= (use_per_token_quant ? m : 1) && k % 8 == 0 && k <= 16384 && m <= INT32_MAX,
              "rms_norm_general: out of input's size, weight / bias [hidden], one scale per token, hidden % 8 == 0 and hidden <= 16384 are required");
  c10::hip::OptionalHIPGuardMasqueradingAsCUDA guard(input.device());
  raise_on(awq_layernorm_quant(input.data_ptr(), weight.data_ptr(), has_bias ? bias->data_ptr() : nullptr, (float)epsilon, out.data_ptr(),
                               scaling.data_ptr(), (int)m, (int)k, use_per_token_quant ? 1 : 0, dtype_code(input),
                               (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream()));
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X-native W4A16 kernels behind llm-awq's awq_inference_engine API (hot path only)";
  m.def("gemm_forward_cuda_new", &gemm_forward_cuda_new, "New quantized GEMM kernel.");
  m.def("gemv_forward_cuda_new", &gemv_forward_cuda_new, "New quantized GEMV kernel.");
  m.def("layernorm_forward_cuda", &layernorm_forward_cuda, "FT RMSNorm into `out` (tinychat's FTLlamaRMSNorm)", py::arg("_input"),
        py::arg("_gamma"), py::arg("_out"), py::arg("eps"));
  m.def("single_query_attention", &single_query_attention, "Attention with a single query", py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("length_per_sample_"), py::arg("alibi_slopes_"), py::arg("timestep"),
        py::arg("rotary_embedding_dim") = 0, py::arg("rotary_base") = 10000.0f, py::arg("rotary_scale") = 1.0f,
        py::arg("neox_rotary_style") = true);
  m.def("attn_prefill", &attn_prefill, "Prefill attention (flash_attn_func's forward): q [B, Sq, H, Dh], k / v [B, Sk, Hkv, Dh]", py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("rope_kv_store", &rope_kv_store, "Rotate q and k of a fused qkv chunk, store k / v into the FT caches; returns q [B, S, H, Dh]", py::arg("qkv"),
        py::arg("freqs"), py::arg("k_cache"), py::arg("v_cache"), py::arg("start_pos"), py::arg("nheads"), py::arg("nheads_kv"));
  m.def("attn_prefill_ftcache", &attn_prefill_ftcache, "Prefill attention with K / V read from the FT caches at positions kv_start .. kv_start + seqlen_k",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("kv_start"), py::arg("seqlen_k"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_splitkv", &attn_splitkv, "attn_prefill on the split-KV kernel pair where attn_splitkv_plan splits (few query rows, long history)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_splitkv_plan", &attn_splitkv_plan, "(splits, chunk) of the split-KV attention plan; splits == 1: the one-pass kernel serves",
        py::arg("batch"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("head_dim"), py::arg("seqlen_q"), py::arg("seqlen_k"), py::arg("causal"));
  m.def("rope_kv_store_natural", &rope_kv_store_natural,
        "Rotate q and k of a fused qkv chunk, store k / v into natural-layout caches [Bc, Lmax, Hkv, Dh]; returns q [B, S, H, Dh]", py::arg("qkv"),
        py::arg("freqs"), py::arg("k_cache"), py::arg("v_cache"), py::arg("start_pos"), py::arg("nheads"), py::arg("nheads_kv"));
  m.def("rope_kv_store_natural_fp8", &rope_kv_store_natural_fp8,
        "rope_kv_store_natural on the FP8 cache: k / v stored as e4m3 codes [Bc, Lmax, Hkv, Dh] with fp32 scales [Bc, Lmax, Hkv]; returns q", py::arg("qkv"),
        py::arg("freqs"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("start_pos"), py::arg("nheads"),
        py::arg("nheads_kv"));
  m.def("attn_prefill_kv8", &attn_prefill_kv8, "attn_prefill with k / v read from e4m3 codes and per-(key, KV head) fp32 scales", py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("k_scale"), py::arg("v_scale"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_splitkv_kv8", &attn_splitkv_kv8, "attn_splitkv with k / v read from e4m3 codes and per-(key, KV head) fp32 scales", py::arg("q"),
        py::arg("k"), py::arg("v"), py::arg("k_scale"), py::arg("v_scale"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("rope_kv_store_natural_pos", &rope_kv_store_natural_pos,
        "rope_kv_store_natural with positions read on the device: cache_seqlens int32 [B], freqs_table [P, rot_dim] the whole angle table",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cache_seqlens"), py::arg("nheads"),
        py::arg("nheads_kv"));
  m.def("rope_kv_store_natural_pos_fp8", &rope_kv_store_natural_pos_fp8, "rope_kv_store_natural_pos on the FP8 cache", py::arg("qkv"),
        py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("cache_seqlens"),
        py::arg("nheads"), py::arg("nheads_kv"));
  m.def("attn_kvcache", &attn_kvcache,
        "Split-KV attention over natural-layout caches with per-sequence lengths seqlens_k[b] + seqlen_offset read on the device", py::arg("q"),
        py::arg("k_cache"), py::arg("v_cache"), py::arg("seqlens_k"), py::arg("max_seqlen_k"), py::arg("seqlen_offset"), py::arg("softmax_scale"),
        py::arg("causal"));
  m.def("attn_kvcache_kv8", &attn_kvcache_kv8, "attn_kvcache with the caches read from e4m3 codes and per-(key, KV head) fp32 scales",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("seqlen_offset"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_kvcache_plan", &attn_kvcache_plan, "(splits, chunk) of attn_kvcache, made from the bound max_seqlen_k alone", py::arg("batch"),
        py::arg("nheads"), py::arg("nheads_kv"), py::arg("head_dim"), py::arg("seqlen_q"), py::arg("max_seqlen_k"));
  m.def("rope_kv_store_paged_pos", &rope_kv_store_paged_pos,
        "rope_kv_store_natural_pos over a paged KV cache: pools [num_pages, page_size, Hkv, Dh], block_table int32 [B, pages_per_seq]",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("block_table"), py::arg("cache_seqlens"),
        py::arg("nheads"), py::arg("nheads_kv"));
  m.def("rope_kv_store_paged_pos_fp8", &rope_kv_store_paged_pos_fp8, "rope_kv_store_paged_pos on FP8 pools", py::arg("qkv"),
        py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"),
        py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"));
  m.def("attn_kvcache_paged", &attn_kvcache_paged,
        "attn_kvcache over a paged KV cache: K / V fetched from pools [num_pages, page_size, Hkv, Dh] through block_table [B, pages_per_seq]",
        py::arg("q"), py::arg("k_pool"), py::arg("v_pool"), py::arg("block_table"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("seqlen_offset"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_kvcache_paged_kv8", &attn_kvcache_paged_kv8, "attn_kvcache_paged on FP8 pools with per-(key, KV head) fp32 scale pools",
        py::arg("q"), py::arg("k_pool"), py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("seqlen_offset"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_kvcache_paged_shared", &attn_kvcache_paged_shared,
        "attn_kvcache_paged for groups of sequences that share a prefix: the prefix keys are fetched once per group",
        py::arg("q"), py::arg("k_pool"), py::arg("v_pool"), py::arg("block_table"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("group_members"), py::arg("group_prefix"), py::arg("seq_prefix"), py::arg("max_prefix"), py::arg("seqlen_offset"),
        py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_kvcache_paged_shared_kv8", &attn_kvcache_paged_shared_kv8, "attn_kvcache_paged_shared on FP8 pools with fp32 scale pools",
        py::arg("q"), py::arg("k_pool"), py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("group_members"), py::arg("group_prefix"), py::arg("seq_prefix"), py::arg("max_prefix"),
        py::arg("seqlen_offset"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("kv_page_copy", &kv_page_copy, "Copy pages of a paged KV cache inside the pools: page dst_pages[i] := page src_pages[i]", py::arg("k_pool"),
        py::arg("v_pool"), py::arg("src_pages"), py::arg("dst_pages"));
  m.def("kv_page_copy_fp8", &kv_page_copy_fp8, "kv_page_copy on FP8 pools and their scale pools", py::arg("k_pool"), py::arg("v_pool"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("src_pages"), py::arg("dst_pages"));
  m.def("attn_prefill_kvcache", &attn_prefill_kvcache,
        "The one-pass prefill kernel over natural-layout caches with per-sequence lengths read on the device: a prompt chunk of any length",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("seqlens_k"), py::arg("max_seqlen_k"), py::arg("seqlen_offset"),
        py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_prefill_kvcache_kv8", &attn_prefill_kvcache_kv8, "attn_prefill_kvcache on the FP8 cache", py::arg("q"), py::arg("k_cache"),
        py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("seqlens_k"), py::arg("max_seqlen_k"), py::arg("seqlen_offset"),
        py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_prefill_paged", &attn_prefill_paged,
        "attn_prefill_kvcache over a paged KV cache: K / V fetched from pools [num_pages, page_size, Hkv, Dh] through block_table [B, pages_per_seq]",
        py::arg("q"), py::arg("k_pool"), py::arg("v_pool"), py::arg("block_table"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("seqlen_offset"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("attn_prefill_paged_kv8", &attn_prefill_paged_kv8, "attn_prefill_paged on FP8 pools with per-(key, KV head) fp32 scale pools", py::arg("q"),
        py::arg("k_pool"), py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("seqlen_offset"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("rope_kv_store_natural_varq", &rope_kv_store_natural_varq,
        "rope_kv_store_natural_pos over PACKED tokens: qkv [total_q, (H + 2 Hkv) Dh], sequence b owns rows cu_seqlens_q[b] .. cu_seqlens_q[b + 1] - 1",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"),
        py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_out") = py::none());
  m.def("rope_kv_store_natural_varq_fp8", &rope_kv_store_natural_varq_fp8, "rope_kv_store_natural_varq on the FP8 cache", py::arg("qkv"),
        py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("cu_seqlens_q"),
        py::arg("max_seqlen_q"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_out") = py::none());
  m.def("rope_kv_store_paged_varq", &rope_kv_store_paged_varq, "rope_kv_store_natural_varq over a paged KV cache", py::arg("qkv"),
        py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"),
        py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_out") = py::none());
  m.def("rope_kv_store_paged_varq_fp8", &rope_kv_store_paged_varq_fp8, "rope_kv_store_paged_varq on FP8 pools", py::arg("qkv"),
        py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"),
        py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"),
        py::arg("q_out") = py::none());
  m.def("rope_kv_store_natural_qknorm", &rope_kv_store_natural_qknorm, "rope_kv_store_natural with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs"), py::arg("k_cache"), py::arg("v_cache"), py::arg("start_pos"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"));
  m.def("rope_kv_store_natural_fp8_qknorm", &rope_kv_store_natural_fp8_qknorm, "rope_kv_store_natural_fp8 with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("start_pos"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"));
  m.def("rope_kv_store_natural_pos_qknorm", &rope_kv_store_natural_pos_qknorm, "rope_kv_store_natural_pos with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"));
  m.def("rope_kv_store_natural_pos_fp8_qknorm", &rope_kv_store_natural_pos_fp8_qknorm, "rope_kv_store_natural_pos_fp8 with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"));
  m.def("rope_kv_store_paged_pos_qknorm", &rope_kv_store_paged_pos_qknorm, "rope_kv_store_paged_pos with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("block_table"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"));
  m.def("rope_kv_store_paged_pos_fp8_qknorm", &rope_kv_store_paged_pos_fp8_qknorm, "rope_kv_store_paged_pos_fp8 with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"));
  m.def("rope_kv_store_natural_varq_qknorm", &rope_kv_store_natural_varq_qknorm, "rope_kv_store_natural_varq with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"), py::arg("q_out") = py::none());
  m.def("rope_kv_store_natural_varq_fp8_qknorm", &rope_kv_store_natural_varq_fp8_qknorm, "rope_kv_store_natural_varq_fp8 with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"), py::arg("v_scale"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"), py::arg("q_out") = py::none());
  m.def("rope_kv_store_paged_varq_qknorm", &rope_kv_store_paged_varq_qknorm, "rope_kv_store_paged_varq with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"), py::arg("q_out") = py::none());
  m.def("rope_kv_store_paged_varq_fp8_qknorm", &rope_kv_store_paged_varq_fp8_qknorm, "rope_kv_store_paged_varq_fp8 with the per-head q/k RMSNorm (gammas float32 [Dh]) in front of the rotation",
        py::arg("qkv"), py::arg("freqs_table"), py::arg("k_pool"), py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("cache_seqlens"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("q_gamma"), py::arg("k_gamma"), py::arg("norm_eps"), py::arg("q_out") = py::none());
  m.def("attn_prefill_varq", &attn_prefill_varq,
        "The one-pass prefill kernel over PACKED queries q [total_q, H, Dh] with per-sequence query lengths (cu_seqlens_q) and key lengths on the device",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_prefill_varq_kv8", &attn_prefill_varq_kv8, "attn_prefill_varq on the FP8 cache", py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_prefill_paged_varq", &attn_prefill_paged_varq, "attn_prefill_varq over a paged KV cache", py::arg("q"), py::arg("k_pool"),
        py::arg("v_pool"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_prefill_paged_varq_kv8", &attn_prefill_paged_varq_kv8, "attn_prefill_paged_varq on FP8 pools", py::arg("q"), py::arg("k_pool"),
        py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"),
        py::arg("seqlens_k"), py::arg("max_seqlen_k"), py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"),
        py::arg("out") = py::none());
  m.def("attn_varq", &attn_varq,
        "A mixed packed step: attn_prefill_varq with the sequences of at most split_seqlen_q new tokens over at least split_min_keys keys served by the split-KV pair",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("lens_before_step"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_varq_kv8", &attn_varq_kv8, "attn_varq on the FP8 cache", py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("k_scale"),
        py::arg("v_scale"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"),
        py::arg("out") = py::none());
  m.def("attn_paged_varq", &attn_paged_varq, "attn_varq over a paged KV cache", py::arg("q"), py::arg("k_pool"), py::arg("v_pool"),
        py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"),
        py::arg("out") = py::none());
  m.def("attn_paged_varq_kv8", &attn_paged_varq_kv8, "attn_paged_varq on FP8 pools", py::arg("q"), py::arg("k_pool"), py::arg("v_pool"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("lens_before_step"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_varq_window", &attn_varq_window, "attn_varq with a sliding window: a row attends its own key and the window_left keys before it",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"), py::arg("lens_before_step"),
        py::arg("softmax_scale"), py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_varq_window_kv8", &attn_varq_window_kv8, "attn_varq_window on the FP8 cache", py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"), py::arg("lens_before_step"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_paged_varq_window", &attn_paged_varq_window, "attn_varq_window over a paged KV cache", py::arg("q"), py::arg("k_pool"),
        py::arg("v_pool"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"), py::arg("lens_before_step"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_paged_varq_window_kv8", &attn_paged_varq_window_kv8, "attn_paged_varq_window on FP8 pools", py::arg("q"), py::arg("k_pool"),
        py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"),
        py::arg("seqlens_k"), py::arg("max_seqlen_k"), py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"),
        py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_varq_softcap", &attn_varq_softcap, "attn_varq_window with the logits capped: softcap * tanh(scale * q.k / softcap) in front of the mask",
        py::arg("q"), py::arg("k_cache"), py::arg("v_cache"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"),
        py::arg("max_seqlen_k"), py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"), py::arg("softcap"), py::arg("lens_before_step"),
        py::arg("softmax_scale"), py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_varq_softcap_kv8", &attn_varq_softcap_kv8, "attn_varq_softcap on the FP8 cache", py::arg("q"), py::arg("k_cache"), py::arg("v_cache"),
        py::arg("k_scale"), py::arg("v_scale"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"), py::arg("softcap"), py::arg("lens_before_step"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_paged_varq_softcap", &attn_paged_varq_softcap, "attn_varq_softcap over a paged KV cache", py::arg("q"), py::arg("k_pool"),
        py::arg("v_pool"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"), py::arg("seqlens_k"), py::arg("max_seqlen_k"),
        py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"), py::arg("softcap"), py::arg("lens_before_step"), py::arg("softmax_scale"),
        py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_paged_varq_softcap_kv8", &attn_paged_varq_softcap_kv8, "attn_paged_varq_softcap on FP8 pools", py::arg("q"), py::arg("k_pool"),
        py::arg("v_pool"), py::arg("k_scale"), py::arg("v_scale"), py::arg("block_table"), py::arg("cu_seqlens_q"), py::arg("max_seqlen_q"),
        py::arg("seqlens_k"), py::arg("max_seqlen_k"), py::arg("split_seqlen_q"), py::arg("split_min_keys"), py::arg("window_left"), py::arg("softcap"),
        py::arg("lens_before_step"), py::arg("softmax_scale"), py::arg("causal"), py::arg("out") = py::none());
  m.def("attn_varq_window_plan", &attn_varq_window_plan,
        "(splits, chunk) of the split pair of a windowed mixed step: attn_kvcache_plan's for min(max_seqlen_k, window_left + split_seqlen_q + 63)",
        py::arg("batch"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("head_dim"), py::arg("split_seqlen_q"), py::arg("max_seqlen_k"),
        py::arg("window_left"));
  m.def("attn_varq_split_plan", &attn_varq_split_plan, "(splits, chunk) of the split pair of a mixed step: attn_kvcache_plan's for the same bound",
        py::arg("batch"), py::arg("nheads"), py::arg("nheads_kv"), py::arg("head_dim"), py::arg("split_seqlen_q"), py::arg("max_seqlen_k"));
  m.def("attn_varq_plan", &attn_varq_plan, "(q_tile_rows, blocks) of a packed-query launch: a provisional host rule", py::arg("batch"),
        py::arg("nheads"), py::arg("nheads_kv"), py::arg("head_dim"), py::arg("max_seqlen_q"));
  m.def("attn_varlen_qkvpacked", &attn_varlen_qkvpacked,
        "Encoder attention over packed sequences (flash_attn_varlen_qkvpacked_func's forward): qkv [nnz, 3, H, Dh], cu_seqlens int32 [nseq + 1]",
        py::arg("qkv"), py::arg("cu_seqlens"), py::arg("max_seqlen"), py::arg("softmax_scale"), py::arg("causal"));
  m.def("rotary_embedding_neox", &rotary_embedding_neox, "Apply GPT-NeoX style rotary embedding to query and key");
  m.def("fused_rope_with_pos_forward_func", &fused_rope_with_pos_forward_func, "Fused rope forward function with B,S,D embedding");
  m.def("w8a8_gemm_forward_cuda", &w8a8_gemm_forward_cuda, "our w8a8 gemm kernel");
  m.def("w8a8_gemm_fuse_bias_forward_cuda", &w8a8_gemm_fuse_bias_forward_cuda, "our w8a8 gemm fused bias kernel");
  m.def("invoke_quant", &invoke_quant, "fp16->int8 quantization");
  m.def("rms_norm_general", &rms_norm_general, py::arg("out"), py::arg("input"), py::arg("weight"), py::arg("bias"), py::arg("scaling"),
        py::arg("epsilon"), py::arg("use_per_token_quant") = true, "LayerNorm (mean subtracted) + int8 quantisation (TRTLLM kernel).");
  m.def("gelu_and_quant", &gelu_and_quant, "Apply gelu act and quant output");
  m.def("abi_version", []() { return awq_abi_version(); });
  m.def("cdna4_cache_info", []() {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    return py::dict(py::arg("enabled") = cache_enabled(), py::arg("entries") = (int64_t)g_cache.size(), py::arg("hits") = g_cache_hits,
                    py::arg("builds") = g_cache_builds, py::arg("sz_builds") = g_cache_sz_builds, py::arg("bytes") = g_cache_bytes,
                    py::arg("inplace") = g_cache_inplace == 1);
  }, "state of the lazy v2 -> cdna4 weight cache behind gemv/gemm_forward_cuda_new");
  auto clear_all = []() {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    while (!g_cache.empty()) {
      restore_inplace(g_cache.begin()->second);  // (in-place entries: the qweight gets its v2 interleave back)
      drop_entry(g_cache.begin());
    }
  };
  m.def("cdna4_cache_clear", clear_all);
  m.def("cdna4_cache_enable", [clear_all](bool on) {
    if (!on) clear_all();  // with the cache off the reference-layout kernels read the qweights: none may stay converted in place
    g_cache_enabled = on ? 1 : 0;
  });
  m.def("cdna4_cache_inplace", [clear_all](bool on) {
    cache_enabled();
    clear_all();
    g_cache_inplace = on ? 1 : 0;
  }, "AWQ_CDNA4_INPLACE at run time: convert qweights where they lie (no second copy) on their first call through the reference entry points");
  m.def("cdna4_restore", [](torch::Tensor kernel) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    auto it = g_cache.find(kernel.data_ptr());
    if (it == g_cache.end()) return false;
    const bool was = it->second.inplace_intact();  // (overwritten since the conversion: the buffer holds v2 data, nothing is restored)
    restore_inplace(it->second);
    drop_entry(it);
    return was;
  }, "undo an in-place conversion of this qweight (e.g. before saving a reference-layout checkpoint); true if it was converted");
  m.def("decode_cdna4_plan", [](int m, int n, int k, int epilogue) {
    int kernel = 0;
    const int passes = awq_w4a16_decode_cdna4_plan(m, n, k, epilogue, &kernel);
    return py::make_tuple(passes, kernel);
  }, "host-side: (weight passes, kernel) of decode_cdna4 for this shape; passes == 0: the shape is not served (use forward_cdna4)");
  m.def("cdna4_is_converted", [](torch::Tensor kernel) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    return kernel.is_cuda() && inplace_converted_locked(kernel);
  }, "true while this qweight's storage holds the cdna4 interleave because the cache converted it in place (AWQ_CDNA4_INPLACE): the module's "
     "`layout` attribute still says v2 -- format tools must cdna4_restore() it before they slice, repack or save it");
  // extras of the MI355X build (not part of the reference module)
  m.def("repack_v2_to_cdna4", &repack_v2_to_cdna4, "qweight v2 -> cdna4 interleave (same shape)");
  m.def("repack_cdna4_to_v2", &repack_cdna4_to_v2, "qweight cdna4 -> v2 interleave (same shape)");
  m.def("pack_sz_cdna4", &pack_sz_cdna4, "scales/scaled_zeros [Gpad,N] -> packed int32 [N/16, K/128, 16]");
  m.def("forward_cdna4", &forward_cdna4, "WQLinear forward on cdna4-interleaved buffers", py::arg("in_feats"),
        py::arg("kernel"), py::arg("scales"), py::arg("zeros"), py::arg("sz_packed"), py::arg("bias") = py::none(), py::arg("sz_half") = py::none());
  m.def("moe_gemm_forward", &moe_gemm_forward, "grouped per-expert W4A16 GEMM (tokens sorted by expert)", py::arg("x_sorted"),
        py::arg("kernel"), py::arg("scales"), py::arg("zeros"), py::arg("expert_offsets"), py::arg("cdna4") = false);
  m.def("moe_forward_cdna4", &moe_forward_cdna4, "grouped per-expert forward on cdna4 buffers (GEMV for <= 8 rows, GEMM otherwise)");
  m.def("moe_route", &moe_route, "router logits [T, E] -> (topk_ids, topk_w, order, inv, offsets): top-k gate + stable sort by expert, one launch",
        py::arg("router_logits"), py::arg("top_k"), py::arg("renormalize") = true);
  m.def("moe_gather", &moe_gather, "xs[r] = x[order[r] / top_k]", py::arg("x"), py::arg("order"), py::arg("top_k"));
  m.def("moe_combine", &moe_combine, "out[t] = sum_j ys[inv[t k + j]] * w[t, j] (fp32 sum of T-rounded products, one final rounding)", py::arg("ys"),
        py::arg("inv"), py::arg("topk_w"));
  m.def("sample_logits", &sample_logits, "logits [B, V], u [B] -> next tokens int32 [B]: temperature, repetition penalty, top-p, top-k and the draw, one launch",
        py::arg("logits"), py::arg("u"), py::kw_only(), py::arg("temperature") = py::none(), py::arg("top_k") = py::none(),
        py::arg("top_p") = py::none(), py::arg("repetition_penalty") = py::none(), py::arg("history") = py::none(),
        py::arg("hist_len") = py::none(), py::arg("seqlens") = py::none(), py::arg("stop_ids") = py::none(), py::arg("finished") = py::none(),
        py::arg("max_len") = 0, py::arg("append") = false, py::arg("advance") = false);
  m.def("spec_draft_ngram", &spec_draft_ngram, "prompt-lookup drafter over the sampler's history -> (drafts int32 [B, kmax], draft_len int32 [B])",
        py::arg("history"), py::arg("hist_len"), py::arg("seqlens"), py::kw_only(), py::arg("vocab"), py::arg("kmax"), py::arg("ngram_min") = 1,
        py::arg("ngram_max") = 3, py::arg("max_len") = 2147483647, py::arg("max_draft") = py::none());
  m.def("spec_pack", &spec_pack, "the layout of a speculative step -> (cu_seqlens_q int32 [B + 1], input_ids int32 [total_q]); drafts / draft_len are rewritten",
        py::arg("last_tokens"), py::arg("drafts"), py::arg("draft_len"), py::arg("seqlens"), py::arg("total_q"));
  m.def("spec_verify", &spec_verify, "sample_logits' row routine on every row of a packed step -> row_tokens int32 [total_q]", py::arg("logits"),
        py::arg("u"), py::arg("cu_seqlens_q"), py::arg("input_ids"), py::kw_only(), py::arg("temperature") = py::none(),
        py::arg("top_k") = py::none(), py::arg("top_p") = py::none(), py::arg("repetition_penalty") = py::none(), py::arg("history") = py::none(),
        py::arg("hist_len") = py::none());
  m.def("spec_accept", &spec_accept, "the accepted drafts and the token behind them, each through append / stop / advance -> (out_tokens [B, kmax + 1], num_emitted [B], last_tokens [B])",
        py::arg("row_tokens"), py::arg("input_ids"), py::arg("cu_seqlens_q"), py::arg("kmax"), py::kw_only(), py::arg("history") = py::none(),
        py::arg("hist_len") = py::none(), py::arg("seqlens") = py::none(), py::arg("stop_ids") = py::none(), py::arg("finished") = py::none(),
        py::arg("max_len") = 0, py::arg("append") = false, py::arg("advance") = false);
  m.def("lm_head", &lm_head, "logits [M, V] = rmsnorm(x) @ weight^T (+ bias): final RMSNorm and vocabulary GEMV in one launch, inactive rows (seqlens < 0) untouched",
        py::arg("x"), py::arg("weight"), py::arg("gamma") = py::none(), py::arg("eps") = 0.0, py::arg("bias") = py::none(),
        py::arg("seqlens") = py::none(), py::arg("out") = py::none(), py::arg("out_dtype") = at::kFloat, py::arg("max_blocks") = 0);
  m.def("lm_head_softcap", &lm_head_softcap, "lm_head with the logits capped in the epilogue: softcap * tanh(y / softcap) in fp32 behind the bias",
        py::arg("x"), py::arg("weight"), py::arg("softcap"), py::arg("gamma") = py::none(), py::arg("eps") = 0.0, py::arg("bias") = py::none(),
        py::arg("seqlens") = py::none(), py::arg("out") = py::none(), py::arg("out_dtype") = at::kFloat, py::arg("max_blocks") = 0);
  m.def("logit_softcap_", &logit_softcap_, "existing logits [B, V] (fp32 / bf16 / fp16) capped in place; rows with seqlens < 0 untouched",
        py::arg("logits"), py::arg("softcap"), py::arg("seqlens") = py::none());
  m.def("embed_tokens", &embed_tokens, "out[i] = table[tokens[i]], zeros for an id outside the table (-1 = a finished slot)", py::arg("tokens"),
        py::arg("table"));
  m.def("lm_head_logprobs", &lm_head_logprobs,
        "(logprob, lse, target_logit, argmax) per row of x against weight [V, K]: the LM head fused with log-sum-exp, no logits written; rows whose target "
        "is outside [0, V) are ignored",
        py::arg("x"), py::arg("weight"), py::arg("targets") = py::none(), py::arg("gamma") = py::none(), py::arg("eps") = 0.0,
        py::arg("bias") = py::none(), py::arg("round_logits") = false, py::arg("max_blocks") = 0);
  m.def("lm_head_logprobs_softcap", &lm_head_logprobs_softcap,
        "lm_head_logprobs with every logit capped, softcap * tanh(z / softcap), before the max / sum-exp, the target pick and the argmax",
        py::arg("x"), py::arg("weight"), py::arg("softcap"), py::arg("targets") = py::none(), py::arg("gamma") = py::none(), py::arg("eps") = 0.0,
        py::arg("bias") = py::none(), py::arg("round_logits") = false, py::arg("max_blocks") = 0);
  m.def("token_logprobs", &token_logprobs, "(logprob, lse, argmax) per row of existing logits [B, V] (fp32 / bf16 / fp16)", py::arg("logits"),
        py::arg("targets") = py::none());
  m.def("lora_shrink", &lora_shrink, "multi-LoRA shrink: ws[s, t, :] = x[t, k of split s] @ A_{adapter of t}^T in fp32 (rows without an adapter untouched)",
        py::arg("x"), py::arg("a_pool"), py::arg("adapter_ids"), py::arg("ws"), py::arg("rank"), py::arg("cu_seqlens_q") = py::none(),
        py::arg("max_seqlen_q") = 1);
  m.def("lora_expand", &lora_expand, "multi-LoRA expand: y[t, :] += T(scaling * sum_s ws[s, t, :]) @ B_{adapter of t}^T in place, one rounding",
        py::arg("ws"), py::arg("b_pool"), py::arg("scaling"), py::arg("adapter_ids"), py::arg("y"), py::arg("k"), py::arg("slice_end"),
        py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = 1);
  m.def("lora_expand_gate_up", &lora_expand_gate_up,
        "multi-LoRA expand on the 8 + 8 interleaved gate / up pair fused with the SiLU * mul tail: h = silu(gate + delta) * (up + delta)", py::arg("ws"),
        py::arg("b_pool"), py::arg("scaling"), py::arg("adapter_ids"), py::arg("y2"), py::arg("k"), py::arg("h") = py::none(),
        py::arg("cu_seqlens_q") = py::none(), py::arg("max_seqlen_q") = 1);
  m.def("quantize_pack", &quantize_pack,
        "AWQ group quantiser + packer, one launch: (w_fake, scales, scaled_zeros, zeros, qweight), None where not wanted", py::arg("w"),
        py::arg("col_scale") = py::none(), py::arg("clip_max") = py::none(), py::arg("n_bit") = 4, py::arg("layout") = "cdna4",
        py::arg("want_fake") = false, py::arg("want_scales") = true, py::arg("want_zeros") = false, py::arg("want_qweight") = true);
  m.def("clip_search", &clip_search, "AWQ clip search, one launch: (best_max_val [N, K/128], best_idx int32, err fp32 [N, K/128, n_steps] or None)",
        py::arg("w"), py::arg("x"), py::arg("n_bit") = 4, py::arg("n_grid") = 20, py::arg("n_steps") = 10, py::arg("return_err") = false);
  m.def("pack_w3", &pack_w3, "logical uint8 [N, K] (0..7) -> w3c tiles int16 [N/4, 3K/4]");
  m.def("forward_w3", &forward_w3, "WQLinear forward for w_bit = 3 (w3c tiles)", py::arg("in_feats"), py::arg("kernel"),
        py::arg("scales"), py::arg("zeros"), py::arg("sz_packed"), py::arg("bias") = py::none());
  m.def("pack_szh_cdna4", &pack_szh_cdna4, "scales/scaled_zeros [Gpad,N] -> (sz_half int32 [N/16, K/128, 16], exact)");
  m.def("decode_cdna4", &decode_cdna4, "<= 8 rows on cdna4 weights + sz_half (LDS-DMA streaming kernel)", py::arg("in_feats"),
        py::arg("kernel"), py::arg("sz_half"), py::arg("bias") = py::none(), py::arg("epilogue") = 0);
  m.def("rmsnorm", &rmsnorm, "RMSNorm of every row (layernorm_forward_cuda's arithmetic), one launch", py::arg("in_feats"), py::arg("gamma"), py::arg("eps"));
  m.def("rmsnorm_forward_cdna4", &rmsnorm_forward_cdna4, "RMSNorm fused in front of the decode GEMV (<= 4 rows)", py::arg("in_feats"),
        py::arg("gamma"), py::arg("eps"), py::arg("kernel"), py::arg("sz_packed"), py::arg("bias") = py::none(),
        py::arg("fused_gate_up") = false);
  m.def("mlp_gate_up_forward_cdna4", &mlp_gate_up_forward_cdna4, "silu(x Wg^T) * (x Wu^T) for any row count on the 8 + 8 interleaved gate/up pair",
        py::arg("in_feats"), py::arg("kernel"), py::arg("sz_packed"), py::arg("sz_half") = py::none());
  m.def("mlp_gate_up_cdna4", &mlp_gate_up_cdna4, "silu(x Wg^T) * (x Wu^T) on stacked cdna4 gate/up buffers, <= 8 rows");
}
