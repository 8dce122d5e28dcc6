// PyTorch bindings for the element-wise / multi-tensor HIP kernels.
// Tensor checks live here; the kernels (csrc/kernels/*.hip) see raw pointers only.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>

#include <cmath>
#include <vector>

#include "dla_kernels.h"
#include "dla_bindings.h"
#include "dla_tables.h"

namespace dla {

int dtype_code(const at::Tensor& t) {
  if (t.scalar_type() == at::kFloat) return kF32;
  if (t.scalar_type() == at::kBFloat16) return kBF16;
  TORCH_CHECK(false, "distributed_learning_amd: unsupported dtype ", t.scalar_type(), " (fp32/bf16 only)");
  return -1;
}

hipStream_t current_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.device().index()).stream();
}

void check_dev(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda(), what, " must be a GPU tensor");
  // Elementwise kernels walk raw storage order, so any dense non-overlapping layout works
  // (channels_last conv weights included) as long as all operands share it.
  TORCH_CHECK(t.is_non_overlapping_and_dense(), what, " must be dense (non-overlapping)");
}

// Uploads a host byte blob to a device uint8 tensor (construction time only).
at::Tensor upload(const void* data, size_t bytes, const at::Device& dev) {
  auto host = at::empty({(int64_t)bytes}, at::TensorOptions().dtype(at::kByte));
  std::memcpy(host.data_ptr(), data, bytes);
  return host.to(dev);
}

// ------------------------------------------------------------------------------------------
// SgdTable: one fused multi-tensor SGD launch per step over a fixed parameter set.
// ------------------------------------------------------------------------------------------
class SgdTable {
 public:
  SgdTable(std::vector<at::Tensor> params, std::vector<at::Tensor> grads, std::vector<at::Tensor> moms,
           std::vector<at::Tensor> shadows)
      : params_(std::move(params)), grads_(std::move(grads)), moms_(std::move(moms)), shadows_(std::move(shadows)) {
    TORCH_CHECK(!params_.empty(), "SgdTable: empty parameter list");
    TORCH_CHECK(params_.size() == grads_.size(), "SgdTable: params/grads size mismatch");
    TORCH_CHECK(moms_.empty() || moms_.size() == params_.size(), "SgdTable: momentum list size mismatch");
    TORCH_CHECK(shadows_.empty() || shadows_.size() == params_.size(), "SgdTable: shadow list size mismatch");
    grad_dtype_ = dtype_code(grads_[0]);
    std::vector<SgdEntry> entries;
    std::vector<int32_t> prefix;
    int32_t blocks = 0;
    const int chunk = mt_chunk_elems();
    for (size_t i = 0; i < params_.size(); ++i) {
      auto& p = params_[i];
      check_dev(p, "param");
      check_dev(grads_[i], "grad");
      TORCH_CHECK(p.scalar_type() == at::kFloat, "SgdTable: parameters must be fp32 (master weights)");
      TORCH_CHECK(grads_[i].numel() == p.numel(), "SgdTable: grad numel mismatch");
      TORCH_CHECK(same_layout(grads_[i], p), "SgdTable: grad layout (strides) must match the parameter");
      TORCH_CHECK(dtype_code(grads_[i]) == grad_dtype_, "SgdTable: all grads must share a dtype");
      SgdEntry e{};
      e.param = p.data_ptr<float>();
      e.grad = grads_[i].data_ptr();
      e.momentum = moms_.empty() ? nullptr : moms_[i].data_ptr<float>();
      if (!moms_.empty()) {
        check_dev(moms_[i], "momentum");
        TORCH_CHECK(moms_[i].numel() == p.numel() && moms_[i].scalar_type() == at::kFloat &&
                        same_layout(moms_[i], p),
                    "SgdTable: momentum buffer must be fp32 with the parameter's layout");
      }
      e.param_bf16 = nullptr;
      if (!shadows_.empty()) {
        check_dev(shadows_[i], "bf16 shadow");
        TORCH_CHECK(shadows_[i].scalar_type() == at::kBFloat16 && shadows_[i].numel() == p.numel(), "bad shadow");
        e.param_bf16 = reinterpret_cast<uint16_t*>(shadows_[i].data_ptr());
      }
      e.numel = p.numel();
      if (e.numel == 0) continue;
      entries.push_back(e);
      prefix.push_back(blocks);
      blocks += (int32_t)((e.numel + chunk - 1) / chunk);
    }
    ntensors_ = (int)entries.size();
    nblocks_ = blocks;
    entries_ = upload(entries.data(), entries.size() * sizeof(SgdEntry), params_[0].device());
    prefix_ = upload(prefix.data(), prefix.size() * sizeof(int32_t), params_[0].device());
  }

  void step(double lr, double momentum, double dampening, double weight_decay, bool nesterov, double grad_scale,
            bool first_step) {
    SgdParams hp{(float)lr, (float)momentum, (float)dampening, (float)weight_decay, (float)grad_scale,
                 nesterov ? 1 : 0, first_step ? 1 : 0};
    launch_sgd(reinterpret_cast<const SgdEntry*>(entries_.data_ptr()), reinterpret_cast<const int32_t*>(prefix_.data_ptr()), ntensors_, nblocks_,
               grad_dtype_, !moms_.empty(), hp, current_stream(params_[0]));
  }

  int num_blocks() const { return nblocks_; }

 private:
  std::vector<at::Tensor> params_, grads_, moms_, shadows_;
  at::Tensor entries_, prefix_;
  int ntensors_ = 0, nblocks_ = 0, grad_dtype_ = kF32;
};

// ------------------------------------------------------------------------------------------
// By-value list launches (tensor addresses may change every step).
// ------------------------------------------------------------------------------------------
// Checks shared by the EMA entry points: an average is fp32, dense, on its target's device, with its target's
// element order; omd (1 - decay) is one fp32 on that device.
static void check_ema(const at::Tensor& e, const at::Tensor& target, size_t i, const char* op) {
  check_dev(e, "ema");
  TORCH_CHECK(e.scalar_type() == at::kFloat && e.device() == target.device() && e.numel() == target.numel() &&
                  same_layout(e, target),
              op, ": ema ", i, " must be fp32 on its target's device with the target's numel and layout");
}

static void check_omd(const at::Tensor& omd, const at::Tensor& like, const char* op) {
  check_dev(omd, "omd");
  TORCH_CHECK(omd.scalar_type() == at::kFloat && omd.numel() == 1 && omd.device() == like.device(), op,
              ": omd must be a 1-element fp32 tensor on the tensors' device");
}

// emas == nullptr: the plain update, exactly sgd_step_list.
static void sgd_step_list_impl(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
                               const std::vector<at::Tensor>& moms, const std::vector<at::Tensor>& shadows,
                               const std::vector<at::Tensor>* emas, const at::Tensor* omd, double lr, double momentum,
                               double dampening, double weight_decay, bool nesterov, double grad_scale,
                               bool first_step) {
  TORCH_CHECK(params.size() == grads.size(), "sgd_step_list: params/grads size mismatch");
  TORCH_CHECK(!emas || emas->size() == params.size(), "sgd_step_list: ema list size mismatch");
  TORCH_CHECK(moms.empty() || moms.size() == params.size(), "sgd_step_list: momentum list size mismatch");
  TORCH_CHECK(shadows.empty() || shadows.size() == params.size(), "sgd_step_list: shadow list size mismatch");
  if (params.empty()) return;
  const int gdt = dtype_code(grads[0]);
  const bool use_m = !moms.empty();
  const SgdParams hp{(float)lr, (float)momentum, (float)dampening, (float)weight_decay, (float)grad_scale,
                     nesterov ? 1 : 0, first_step ? 1 : 0};
  // every launch is built, and so every tensor checked, before the first one runs: a bad tensor anywhere
  // in the list raises with nothing updated
  ListBatcher<SgdEntry> lists("sgd_step_list");
  if (emas) check_omd(*omd, grads[0], "sgd_step_list");
  for (size_t i = 0; i < params.size(); ++i) {
    const at::Tensor& p = params[i];
    const at::Tensor& g = grads[i];
    check_dev(p, "param");
    check_dev(g, "grad");
    TORCH_CHECK(p.scalar_type() == at::kFloat && p.device() == g.device(),
                "sgd_step_list: parameters/masters must be fp32 on the gradients' device");
    TORCH_CHECK(g.device() == grads[0].device(), "sgd_step_list: tensor ", i, " is on another device than the list");
    TORCH_CHECK(dtype_code(g) == gdt && same_layout(g, p),
                "sgd_step_list: grad ", i, " must match its parameter's layout and the list's grad dtype");
    SgdEntry e{};
    e.param = p.data_ptr<float>();
    e.grad = g.data_ptr();
    if (use_m) {
      const at::Tensor& m = moms[i];
      check_dev(m, "momentum");
      TORCH_CHECK(m.scalar_type() == at::kFloat && m.device() == g.device() && same_layout(m, p),
                  "sgd_step_list: bad momentum buffer");
      e.momentum = m.data_ptr<float>();
    }
    if (!shadows.empty()) {
      const at::Tensor& s = shadows[i];
      check_dev(s, "bf16 shadow");
      TORCH_CHECK(s.scalar_type() == at::kBFloat16 && s.device() == g.device() && same_layout(s, p),
                  "sgd_step_list: bad shadow");
      e.param_bf16 = reinterpret_cast<uint16_t*>(s.data_ptr());
    }
    if (emas) check_ema((*emas)[i], p, i, "sgd_step_list");
    e.numel = p.numel();
    lists.add(e, emas ? (*emas)[i].data_ptr<float>() : nullptr);
  }
  hipStream_t st = current_stream(grads[0]);
  for (const auto& L : lists.finish()) {
    if (emas) launch_sgd_ema_list(L.list, L.ema, omd->data_ptr<float>(), L.blocks, gdt, use_m, hp, st);
    else launch_sgd_list(L.list, L.blocks, gdt, use_m, hp, st);
  }
}

void sgd_step_list(std::vector<at::Tensor> params, std::vector<at::Tensor> grads, std::vector<at::Tensor> moms,
                   std::vector<at::Tensor> shadows, double lr, double momentum, double dampening, double weight_decay,
                   bool nesterov, double grad_scale, bool first_step) {
  sgd_step_list_impl(params, grads, moms, shadows, nullptr, nullptr, lr, momentum, dampening, weight_decay, nesterov,
                     grad_scale, first_step);
}

// sgd_step_list that also advances emas[i] = fmaf(omd, p_new - emas[i], emas[i]) in the same launches.
void sgd_ema_step_list(std::vector<at::Tensor> params, std::vector<at::Tensor> grads, std::vector<at::Tensor> moms,
                       std::vector<at::Tensor> shadows, std::vector<at::Tensor> emas, at::Tensor omd, double lr,
                       double momentum, double dampening, double weight_decay, bool nesterov, double grad_scale,
                       bool first_step) {
  sgd_step_list_impl(params, grads, moms, shadows, &emas, &omd, lr, momentum, dampening, weight_decay, nesterov,
                     grad_scale, first_step);
}

// emas[i] = fmaf(omd, srcs[i] - emas[i], emas[i]) (update) / targets[i] <-> emas[i] with shadows[i] =
// bf16(new target) (swap): by-value lists, all launches built and checked before the first one runs.
static void ema_list_op(const char* op, const std::vector<at::Tensor>& targets, const std::vector<at::Tensor>& emas,
                        const std::vector<c10::optional<at::Tensor>>& shadows, const at::Tensor* omd) {
  TORCH_CHECK(targets.size() == emas.size(), op, ": target/ema list size mismatch");
  TORCH_CHECK(shadows.empty() || shadows.size() == targets.size(), op, ": shadow list size mismatch");
  if (targets.empty()) return;
  if (omd) check_omd(*omd, targets[0], op);
  ListBatcher<EmaEntry> lists(op);
  for (size_t i = 0; i < targets.size(); ++i) {
    const at::Tensor& x = targets[i];
    check_dev(x, "target");
    TORCH_CHECK(x.scalar_type() == at::kFloat && x.device() == targets[0].device(), op, ": target ", i,
                " must be fp32 on the list's device");
    check_ema(emas[i], x, i, op);
    EmaEntry e{};
    e.target = x.data_ptr<float>();
    e.ema = emas[i].data_ptr<float>();
    if (!shadows.empty() && shadows[i].has_value() && shadows[i]->defined()) {
      const at::Tensor& s = *shadows[i];
      check_dev(s, "bf16 shadow");
      TORCH_CHECK(s.scalar_type() == at::kBFloat16 && s.device() == x.device() && s.numel() == x.numel() &&
                      same_layout(s, x),
                  op, ": bad shadow ", i);
      e.shadow = reinterpret_cast<uint16_t*>(s.data_ptr());
    }
    e.numel = x.numel();
    lists.add(e);
  }
  hipStream_t st = current_stream(targets[0]);
  for (const auto& L : lists.finish()) {
    if (omd) launch_ema_update_list(L.list, L.blocks, omd->data_ptr<float>(), st);
    else launch_ema_swap_list(L.list, L.blocks, st);
  }
}

void ema_update_list(std::vector<at::Tensor> emas, std::vector<at::Tensor> srcs, at::Tensor omd) {
  ema_list_op("ema_update_list", srcs, emas, {}, &omd);
}

void ema_swap_list(std::vector<at::Tensor> targets, std::vector<at::Tensor> emas,
                   std::vector<c10::optional<at::Tensor>> shadows) {
  ema_list_op("ema_swap_list", targets, emas, shadows, nullptr);
}

// ------------------------------------------------------------------------------------------
// Fused LARS / tensor-list L2 norms. LarsPlan owns what is static for one set of participating
// tensors: the device table (partial ranges, group, hyper-parameters) and the workspace. A step
// is square-sum launches, one finalize, update launches; nothing is read back to the host.
// ------------------------------------------------------------------------------------------
class LarsPlan {
 public:
  LarsPlan(std::vector<int64_t> numels, std::vector<int64_t> groups, std::vector<bool> adapt,
           std::vector<double> weight_decay, std::vector<double> eta, std::vector<double> eps,
           std::vector<double> momentum, c10::optional<at::Tensor> lr_dev, at::Tensor like)
      : numels_(std::move(numels)) {
    const size_t T = numels_.size();
    TORCH_CHECK(T > 0 && T < (size_t)1 << 24, "LarsPlan: bad tensor count ", T);
    TORCH_CHECK(groups.size() == T && adapt.size() == T && weight_decay.size() == T && eta.size() == T &&
                    eps.size() == T && momentum.size() == T,
                "LarsPlan: per-tensor lists must have one entry per tensor");
    TORCH_CHECK(like.is_cuda(), "LarsPlan: GPU tensors only");
    int64_t ngroups = 1;
    if (lr_dev.has_value() && lr_dev->defined()) {
      check_dev(*lr_dev, "lr_dev");
      TORCH_CHECK(lr_dev->scalar_type() == at::kFloat && lr_dev->device() == like.device() && lr_dev->is_contiguous(),
                  "LarsPlan: lr_dev must be a contiguous fp32 tensor on the parameters' device");
      lr_dev_ = *lr_dev;
      ngroups = lr_dev_.numel();
    }
    const int chunk = mt_chunk_elems();
    std::vector<LarsTensor> rows(T);
    int64_t blocks = 0;
    for (size_t i = 0; i < T; ++i) {
      TORCH_CHECK(numels_[i] >= 0, "LarsPlan: negative numel");
      TORCH_CHECK(groups[i] >= 0 && groups[i] < ngroups, "LarsPlan: group ", groups[i], " out of range");
      LarsTensor& r = rows[i];
      r.part_begin = (int32_t)blocks;
      blocks += (numels_[i] + chunk - 1) / chunk;
      TORCH_CHECK(blocks < ((int64_t)1 << 30), "LarsPlan: too many chunks");
      r.part_end = (int32_t)blocks;
      r.group = (int32_t)groups[i];
      r.adapt = adapt[i] ? 1 : 0;
      r.weight_decay = adapt[i] ? (float)weight_decay[i] : 0.f;
      r.eta = (float)eta[i];
      r.eps = (float)eps[i];
      r.momentum = (float)momentum[i];
    }
    nblocks_ = (int)blocks;
    table_ = upload(rows.data(), rows.size() * sizeof(LarsTensor), like.device());
    ws_ = at::empty({lars_ws_floats((int)T, nblocks_)}, like.options().dtype(at::kFloat));
  }

  int ntensors() const { return (int)numels_.size(); }
  const LarsTensor* table() const { return reinterpret_cast<const LarsTensor*>(table_.data_ptr()); }
  float* ws() const { return ws_.data_ptr<float>(); }
  at::Tensor grad_norm() const { return ws_.narrow(0, 1, 1); }
  at::Tensor local_lr() const { return ws_.narrow(0, kLarsHead, ntensors()); }
  // [T, 2]: (||p_t||, ||g_t||), the gradient norm before grad_scale and clipping
  at::Tensor norms() const { return ws_.narrow(0, kLarsHead + ntensors(), 2 * (int64_t)ntensors()).view({-1, 2}); }

  // params may be empty (norms of `grads` only); moms / shadows are used by the update pass alone.
  void run(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
           const std::vector<at::Tensor>& moms, const std::vector<c10::optional<at::Tensor>>& shadows, bool update,
           double grad_scale, double max_grad_norm, const std::vector<at::Tensor>* emas = nullptr,
           const at::Tensor* omd = nullptr) {
    const size_t T = numels_.size();
    TORCH_CHECK(!emas || (update && emas->size() == T), "lars: ema list size mismatch");
    if (emas) check_omd(*omd, ws_, "lars");
    TORCH_CHECK(grads.size() == T, "lars: the plan was built for ", T, " tensors, got ", grads.size());
    TORCH_CHECK(params.empty() || params.size() == T, "lars: params/grads size mismatch");
    TORCH_CHECK(!update || (params.size() == T && moms.size() == T && lr_dev_.defined()),
                "lars: the update needs a parameter and a momentum buffer per gradient, and lr_dev");
    TORCH_CHECK(shadows.empty() || shadows.size() == T, "lars: shadow list size mismatch");
    // the launches of both passes, built once: by-value lists split at kMaxList tensors and at grad dtype changes;
    // empty tensors keep their slot, so that slot t of a launch is table row tensor_base + t
    ListBatcher<SgdEntry> lists("lars", /*keep_empty=*/true);
    for (size_t i = 0; i < T; ++i) {
      const at::Tensor& g = grads[i];
      check_dev(g, "grad");
      TORCH_CHECK(g.device() == ws_.device(), "lars: tensor ", i, " is on another device than the plan");
      TORCH_CHECK(g.numel() == numels_[i], "lars: tensor ", i, " has ", g.numel(), " elements, the plan ", numels_[i]);
      lists.tag(dtype_code(g));
      SgdEntry e{};
      float* ema = nullptr;
      e.grad = g.data_ptr();
      e.numel = g.numel();
      if (!params.empty()) {
        const at::Tensor& p = params[i];
        check_dev(p, "param");
        TORCH_CHECK(p.scalar_type() == at::kFloat && p.device() == g.device(),
                    "lars: parameters/masters must be fp32 on the gradients' device");
        TORCH_CHECK(same_layout(g, p), "lars: grad ", i, " must match its parameter's layout");
        e.param = p.data_ptr<float>();
      }
      if (update) {
        const at::Tensor& m = moms[i];
        check_dev(m, "momentum");
        TORCH_CHECK(m.scalar_type() == at::kFloat && m.device() == g.device() && same_layout(m, params[i]),
                    "lars: bad momentum buffer");
        e.momentum = m.data_ptr<float>();
        if (!shadows.empty() && shadows[i].has_value() && (*shadows[i]).defined()) {
          const at::Tensor& s = *shadows[i];
          check_dev(s, "bf16 shadow");
          TORCH_CHECK(s.scalar_type() == at::kBFloat16 && s.device() == g.device() && same_layout(s, params[i]),
                      "lars: bad shadow");
          e.param_bf16 = reinterpret_cast<uint16_t*>(s.data_ptr());
        }
        if (emas) {
          check_ema((*emas)[i], params[i], i, "lars");
          ema = (*emas)[i].data_ptr<float>();
        }
      }
      lists.add(e, ema);
    }
    const auto& launches = lists.finish();
    TORCH_CHECK(lists.total_blocks() == nblocks_, "lars: chunk count changed since the plan was built");
    hipStream_t st = current_stream(ws_);
    for (const auto& L : launches)
      launch_sqsum_list({L.list, L.tensor_base, L.block_base}, L.blocks, L.tag, ws(), (int)T, st);
    launch_lars_finalize(table(), (int)T, lr_dev_.defined() ? lr_dev_.data_ptr<float>() : nullptr, (float)grad_scale,
                         (float)max_grad_norm, ws(), st);
    if (update)
      for (const auto& L : launches) {
        const LarsList list{L.list, L.tensor_base, L.block_base};
        if (emas) launch_lars_ema_list(list, L.ema, omd->data_ptr<float>(), L.blocks, L.tag, table(), ws(), st);
        else launch_lars_list(list, L.blocks, L.tag, table(), ws(), st);
      }
    launches_ = (int)launches.size() * (update ? 2 : 1) + 1;
  }

  int last_launches() const { return launches_; }

 private:
  std::vector<int64_t> numels_;
  at::Tensor table_, ws_, lr_dev_;
  int nblocks_ = 0, launches_ = 0;
};

void lars_step_list(LarsPlan& plan, std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                    std::vector<at::Tensor> moms, std::vector<c10::optional<at::Tensor>> shadows, double grad_scale,
                    double max_grad_norm) {
  plan.run(params, grads, moms, shadows, true, grad_scale, max_grad_norm);
}

// lars_step_list that also advances emas[i] from the fp32 value the update stores, in the update launches.
void lars_ema_step_list(LarsPlan& plan, std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                        std::vector<at::Tensor> moms, std::vector<c10::optional<at::Tensor>> shadows,
                        std::vector<at::Tensor> emas, at::Tensor omd, double grad_scale, double max_grad_norm) {
  plan.run(params, grads, moms, shadows, true, grad_scale, max_grad_norm, &emas, &omd);
}

// ------------------------------------------------------------------------------------------
// Fused LAMB / AdamW (formula and passes: dla_kernels.h). AdamPlan owns what is static for one set of
// participating tensors: the device table (partial ranges, group, hyper-parameters, the address of each
// tensor's int32 update count), the workspace, and for clipping a LARS-layout workspace and table for the
// gradient square sums. Nothing is read back to the host; the finalize launch advances the counts.
// ------------------------------------------------------------------------------------------
class AdamPlan {
 public:
  AdamPlan(bool trust, std::vector<int64_t> numels, std::vector<int64_t> groups, std::vector<bool> adapt,
           std::vector<double> weight_decay, std::vector<double> beta1, std::vector<double> beta2,
           std::vector<double> eps, std::vector<at::Tensor> steps, at::Tensor lr_dev, at::Tensor like)
      : trust_(trust), numels_(std::move(numels)), steps_(std::move(steps)) {
    const size_t T = numels_.size();
    TORCH_CHECK(T > 0 && T < (size_t)1 << 24, "AdamPlan: bad tensor count ", T);
    TORCH_CHECK(groups.size() == T && adapt.size() == T && weight_decay.size() == T && beta1.size() == T &&
                    beta2.size() == T && eps.size() == T && steps_.size() == T,
                "AdamPlan: per-tensor lists must have one entry per tensor");
    TORCH_CHECK(like.is_cuda(), "AdamPlan: GPU tensors only");
    check_dev(lr_dev, "lr_dev");
    TORCH_CHECK(lr_dev.scalar_type() == at::kFloat && lr_dev.device() == like.device() && lr_dev.is_contiguous(),
                "AdamPlan: lr_dev must be a contiguous fp32 tensor on the parameters' device");
    lr_dev_ = lr_dev;
    const int chunk = mt_chunk_elems();
    std::vector<AdamTensor> rows(T);
    std::vector<LarsTensor> clip_rows(T);
    int64_t blocks = 0;
    for (size_t i = 0; i < T; ++i) {
      TORCH_CHECK(numels_[i] >= 0, "AdamPlan: negative numel");
      TORCH_CHECK(groups[i] >= 0 && groups[i] < lr_dev_.numel(), "AdamPlan: group ", groups[i], " out of range");
      TORCH_CHECK(eps[i] > 0 && beta1[i] >= 0 && beta1[i] < 1 && beta2[i] >= 0 && beta2[i] < 1,
                  "AdamPlan: eps > 0 and betas in [0, 1) required");
      check_step(steps_[i], like, i);
      AdamTensor& r = rows[i];
      r.part_begin = (int32_t)blocks;
      blocks += (numels_[i] + chunk - 1) / chunk;
      TORCH_CHECK(blocks < ((int64_t)1 << 30), "AdamPlan: too many chunks");
      r.part_end = (int32_t)blocks;
      r.group = (int32_t)groups[i];
      r.adapt = trust && adapt[i] ? 1 : 0;
      r.weight_decay = (float)weight_decay[i];
      r.eps = (float)eps[i];
      r.beta1 = (float)beta1[i];
      r.beta2 = (float)beta2[i];
      r.omb1 = (float)(1.0 - beta1[i]);
      r.omb2 = (float)(1.0 - beta2[i]);
      r.ln_beta1 = (float)std::log(beta1[i]);
      r.ln_beta2 = (float)std::log(beta2[i]);
      r.step = steps_[i].data_ptr<int32_t>();
      clip_rows[i] = LarsTensor{r.part_begin, r.part_end, 0, 0, 0.f, 0.f, 0.f, 0.f};
    }
    nblocks_ = (int)blocks;
    table_ = upload(rows.data(), rows.size() * sizeof(AdamTensor), like.device());
    clip_table_ = upload(clip_rows.data(), clip_rows.size() * sizeof(LarsTensor), like.device());
    ws_ = at::zeros({adam_ws_floats((int)T, nblocks_)}, like.options().dtype(at::kFloat));
    ws_clip_ = at::zeros({lars_ws_floats((int)T, nblocks_)}, like.options().dtype(at::kFloat));
  }

  bool trust() const { return trust_; }
  int ntensors() const { return (int)numels_.size(); }
  at::Tensor grad_norm() const { return ws_clip_.narrow(0, 1, 1); }  // G of the last step with clipping on
  at::Tensor alpha() const { return ws_.narrow(0, 0, ntensors()); }  // lr * trust
  // [T, 2]: (1 - beta1^k, 1 - beta2^k) of the last step
  at::Tensor bias_corrections() const { return ws_.narrow(0, ntensors(), 2 * (int64_t)ntensors()).view({-1, 2}); }
  // [T, 2]: (||p_t||, ||u_t||) of the last step (LAMB)
  at::Tensor norms() const { return ws_.narrow(0, 3 * (int64_t)ntensors(), 2 * (int64_t)ntensors()).view({-1, 2}); }
  int last_launches() const { return launches_; }

  void run(const std::vector<at::Tensor>& params, const std::vector<at::Tensor>& grads,
           const std::vector<at::Tensor>& ms, const std::vector<at::Tensor>& vs,
           const std::vector<c10::optional<at::Tensor>>& shadows, const std::vector<at::Tensor>& steps,
           double grad_scale, double max_grad_norm, const std::vector<at::Tensor>* emas = nullptr,
           const at::Tensor* omd = nullptr) {
    const char* op = trust_ ? "lamb" : "adamw";
    const size_t T = numels_.size();
    TORCH_CHECK(grads.size() == T, op, ": the plan was built for ", T, " tensors, got ", grads.size());
    TORCH_CHECK(params.size() == T && ms.size() == T && vs.size() == T && steps.size() == T, op,
                ": a parameter, two moments and a step count per gradient are needed");
    TORCH_CHECK(shadows.empty() || shadows.size() == T, op, ": shadow list size mismatch");
    TORCH_CHECK(!emas || emas->size() == T, op, ": ema list size mismatch");
    TORCH_CHECK(max_grad_norm >= 0, op, ": max_grad_norm must be >= 0");
    if (emas) check_omd(*omd, ws_, op);
    // every launch is built, and so every tensor checked, before the first one runs; empty tensors keep their
    // slot, so that slot t of a launch is table row tensor_base + t
    ListBatcher<AdamEntry> lists(op, /*keep_empty=*/true);
    for (size_t i = 0; i < T; ++i) {
      const at::Tensor& g = grads[i];
      const at::Tensor& p = params[i];
      check_dev(g, "grad");
      check_dev(p, "param");
      TORCH_CHECK(g.device() == ws_.device(), op, ": tensor ", i, " is on another device than the plan");
      TORCH_CHECK(g.numel() == numels_[i], op, ": tensor ", i, " has ", g.numel(), " elements, the plan ", numels_[i]);
      TORCH_CHECK(p.scalar_type() == at::kFloat && p.device() == g.device(), op,
                  ": parameters/masters must be fp32 on the gradients' device");
      TORCH_CHECK(same_layout(g, p), op, ": grad ", i, " must match its parameter's layout");
      lists.tag(dtype_code(g));
      AdamEntry e{};
      e.param = p.data_ptr<float>();
      e.grad = g.data_ptr();
      e.numel = g.numel();
      for (int j = 0; j < 2; ++j) {
        const at::Tensor& m = j == 0 ? ms[i] : vs[i];
        check_dev(m, "moment");
        TORCH_CHECK(m.scalar_type() == at::kFloat && m.device() == g.device() && same_layout(m, p), op, ": moment ", i,
                    " must be fp32 on the gradients' device with the parameter's layout");
        (j == 0 ? e.m : e.v) = m.data_ptr<float>();
      }
      if (!shadows.empty() && shadows[i].has_value() && (*shadows[i]).defined()) {
        const at::Tensor& s = *shadows[i];
        check_dev(s, "bf16 shadow");
        TORCH_CHECK(s.scalar_type() == at::kBFloat16 && s.device() == g.device() && same_layout(s, p), op,
                    ": bad shadow");
        e.param_bf16 = reinterpret_cast<uint16_t*>(s.data_ptr());
      }
      check_step(steps[i], ws_, i);
      TORCH_CHECK(steps[i].data_ptr() == steps_[i].data_ptr(), op, ": step count ", i,
                  " is not the tensor the plan was built with");
      float* ema = nullptr;
      if (emas) {
        check_ema((*emas)[i], p, i, op);
        ema = (*emas)[i].data_ptr<float>();
      }
      lists.add(e, ema);
    }
    const auto& launches = lists.finish();
    TORCH_CHECK(lists.total_blocks() == nblocks_, op, ": chunk count changed since the plan was built");
    hipStream_t st = current_stream(ws_);
    const bool clip = max_grad_norm > 0;
    const float gs = (float)grad_scale, mgn = (float)max_grad_norm;
    const AdamTensor* table = reinterpret_cast<const AdamTensor*>(table_.data_ptr());
    float* ws = ws_.data_ptr<float>();
    float* wsc = clip ? ws_clip_.data_ptr<float>() : nullptr;
    const float* lr = lr_dev_.data_ptr<float>();
    const float* omdp = emas ? omd->data_ptr<float>() : nullptr;
    if (clip)  // gradient square sums only: the SgdList of the square-sum kernel with a null parameter
      for (const auto& L : launches) {
        LarsList gl{};
        gl.l.ntensors = L.list.ntensors;
        for (int t = 0; t <= L.list.ntensors; ++t) gl.l.prefix[t] = L.list.prefix[t];
        for (int t = 0; t < L.list.ntensors; ++t) {
          gl.l.e[t].grad = L.list.e[t].grad;
          gl.l.e[t].numel = L.list.e[t].numel;
        }
        gl.tensor_base = L.tensor_base;
        gl.block_base = L.block_base;
        launch_sqsum_list(gl, L.blocks, L.tag, wsc, (int)T, st);
      }
    if (trust_) {
      if (clip)
        launch_lars_finalize(reinterpret_cast<const LarsTensor*>(clip_table_.data_ptr()), (int)T, nullptr, gs, mgn, wsc,
                             st);
      for (const auto& L : launches)
        launch_lamb_moments_list(L.list, L.tensor_base, L.block_base, L.blocks, L.tag, table, wsc, gs, ws, (int)T, st);
      launch_adam_finalize(table, (int)T, lr, true, false, gs, mgn, wsc, ws, st);
      for (const auto& L : launches)
        launch_lamb_apply_list(L.list, L.tensor_base, L.blocks, emas ? &L.ema : nullptr, omdp, table, ws, (int)T, st);
      launches_ = (int)launches.size() * (clip ? 3 : 2) + (clip ? 2 : 1);
    } else {
      launch_adam_finalize(table, (int)T, lr, false, clip, gs, mgn, wsc, ws, st);
      for (const auto& L : launches)
        launch_adamw_list(L.list, L.tensor_base, L.blocks, L.tag, emas ? &L.ema : nullptr, omdp, table, wsc, gs, ws,
                          (int)T, st);
      launches_ = (int)launches.size() * (clip ? 2 : 1) + 1;
    }
  }

 private:
  static void check_step(const at::Tensor& s, const at::Tensor& like, size_t i) {
    TORCH_CHECK(s.is_cuda() && s.device() == like.device() && s.scalar_type() == at::kInt && s.numel() == 1,
                "lamb/adamw: step count ", i, " must be a one-element int32 tensor on the parameters' device");
  }

  bool trust_;
  std::vector<int64_t> numels_;
  std::vector<at::Tensor> steps_;
  at::Tensor table_, clip_table_, ws_, ws_clip_, lr_dev_;
  int nblocks_ = 0, launches_ = 0;
};

// lamb_step_list / adamw_step_list (kTrust: the kind of plan each takes), and their _ema forms, which also advance
// emas[i] from the fp32 value the update stores, in the update launches.
template <bool kTrust>
void adam_step_list(AdamPlan& plan, std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                    std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                    std::vector<c10::optional<at::Tensor>> shadows, std::vector<at::Tensor> steps, double grad_scale,
                    double max_grad_norm) {
  TORCH_CHECK(plan.trust() == kTrust, "lamb/adamw: the plan was built for the other optimizer");
  plan.run(params, grads, ms, vs, shadows, steps, grad_scale, max_grad_norm);
}

template <bool kTrust>
void adam_ema_step_list(AdamPlan& plan, std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                        std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                        std::vector<c10::optional<at::Tensor>> shadows, std::vector<at::Tensor> steps,
                        std::vector<at::Tensor> emas, at::Tensor omd, double grad_scale, double max_grad_norm) {
  TORCH_CHECK(plan.trust() == kTrust, "lamb/adamw: the plan was built for the other optimizer");
  plan.run(params, grads, ms, vs, shadows, steps, grad_scale, max_grad_norm, &emas, &omd);
}

// (per_tensor[T], total[1]) = scale * (||t||_2 of each tensor, of all of them together), fp32.
// A one-off plan per call: a host-built table uploaded synchronously and a fresh workspace that the
// results are views of -- not for the inside of a step or a graph capture (FusedLARS caches its plan).
std::vector<at::Tensor> multi_tensor_l2norm(std::vector<at::Tensor> tensors, double scale) {
  TORCH_CHECK(!tensors.empty(), "multi_tensor_l2norm: empty tensor list");
  const size_t T = tensors.size();
  std::vector<int64_t> numels(T);
  for (size_t i = 0; i < T; ++i) numels[i] = tensors[i].numel();
  LarsPlan plan(numels, std::vector<int64_t>(T, 0), std::vector<bool>(T, false), std::vector<double>(T, 0.0),
                std::vector<double>(T, 0.0), std::vector<double>(T, 0.0), std::vector<double>(T, 0.0), c10::nullopt,
                tensors[0]);
  plan.run({}, tensors, {}, {}, false, scale, 0.0);
  return {plan.norms().select(1, 1).mul(scale), plan.grad_norm()};
}

void pack_tensors_on(const std::vector<at::Tensor>& ts, const std::vector<int64_t>& offs, const at::Tensor& flat,
                     float scale, hipStream_t st) {
  TORCH_CHECK(ts.size() == offs.size(), "pack: tensors/offsets size mismatch");
  const int fdt = dtype_code(flat);
  // as in sgd_step_list: all launches built and checked first, so a bad slot leaves `flat` untouched
  ListBatcher<PackEntry> lists("pack");
  for (size_t i = 0; i < ts.size(); ++i) {
    check_dev(ts[i], "pack tensor");
    lists.tag(dtype_code(ts[i]));  // a launch has one source dtype
    TORCH_CHECK(offs[i] >= 0 && offs[i] + ts[i].numel() <= flat.numel(), "pack: slot ", i, " out of range");
    lists.add(PackEntry{ts[i].data_ptr(), ts[i].numel(), offs[i]});
  }
  for (const auto& L : lists.finish()) launch_pack_list(L.list, L.blocks, L.tag, fdt, flat.data_ptr(), scale, st);
}

void pack_list(std::vector<at::Tensor> ts, std::vector<int64_t> offs, at::Tensor flat, double scale) {
  check_dev(flat, "flat");
  pack_tensors_on(ts, offs, flat, (float)scale, current_stream(flat));
}

// ------------------------------------------------------------------------------------------
// PackTable (declared in dla_tables.h).
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// Free functions
// ------------------------------------------------------------------------------------------
void reduce_sum_(at::Tensor dst, std::vector<at::Tensor> srcs, bool accumulate, double scale) {
  check_dev(dst, "dst");
  TORCH_CHECK((int)srcs.size() <= kMaxReduceSrc, "reduce_sum_: at most ", kMaxReduceSrc, " sources");
  ReduceSrcs rs{};
  rs.count = (int)srcs.size();
  for (size_t i = 0; i < srcs.size(); ++i) {
    check_dev(srcs[i], "src");
    TORCH_CHECK(srcs[i].scalar_type() == dst.scalar_type(), "reduce_sum_: dtype mismatch");
    TORCH_CHECK(srcs[i].numel() >= dst.numel(), "reduce_sum_: source shorter than destination");
    rs.ptr[i] = srcs[i].data_ptr();
  }
  launch_reduce_sum(dst.data_ptr(), accumulate, rs, dst.numel(), dtype_code(dst), (float)scale, current_stream(dst));
}

void scale_(at::Tensor t, double scale) {
  check_dev(t, "tensor");
  launch_scale(t.data_ptr(), t.numel(), dtype_code(t), (float)scale, current_stream(t));
}

static const int64_t* step_ptr(const c10::optional<at::Tensor>& step, const at::Tensor& t) {
  if (!step.has_value() || !step->defined()) return nullptr;
  TORCH_CHECK(step->scalar_type() == at::kLong && step->numel() == 1 && step->device() == t.device(),
              "step must be a one-element int64 tensor on the output's device");
  return step->data_ptr<int64_t>();
}

void uniform_(at::Tensor t, int64_t seed, int64_t offset, double lo, double hi, c10::optional<at::Tensor> step,
              int64_t per_step) {
  check_dev(t, "tensor");
  launch_uniform_fill(t.data_ptr(), t.numel(), dtype_code(t), (uint64_t)seed, (uint64_t)offset, (float)lo, (float)hi,
                      current_stream(t), step_ptr(step, t), (uint64_t)per_step);
}

void randint_(at::Tensor t, int64_t high, int64_t seed, int64_t offset, c10::optional<at::Tensor> step,
              int64_t per_step) {
  check_dev(t, "tensor");
  TORCH_CHECK(t.scalar_type() == at::kLong, "randint_: int64 tensor required");
  TORCH_CHECK(high > 0, "randint_: high must be positive");
  launch_randint_fill(t.data_ptr<int64_t>(), t.numel(), high, (uint64_t)seed, (uint64_t)offset, current_stream(t),
                      step_ptr(step, t), (uint64_t)per_step);
}

// out: logical [N, 3, Ho, Wo] in channels-last memory (dense [N, Ho, Wo, 3]), possibly a slice of a larger
// buffer. Everything is checked before the launch; the kernel indexes elements with 32 bits.
struct AugmentDims {
  int N, Hs, Ws, Ho, Wo, dtype;
};

// The checks the augment bindings share; `op` prefixes the messages. With `index` (the indexed forms) src is a
// store [P, Hs, Ws, 3] of any size, N is out's and index's length and the 2^31 limit applies to one image.
static AugmentDims check_augment_args(const char* op, const at::Tensor& src, const at::Tensor& out,
                                      const at::Tensor& geom, const at::Tensor& flip, const at::Tensor& scale,
                                      const at::Tensor& bias, int64_t pad, const at::Tensor* index = nullptr) {
  TORCH_CHECK(src.is_cuda() && out.is_cuda() && geom.is_cuda() && flip.is_cuda() && scale.is_cuda() && bias.is_cuda(),
              op, ": every tensor must be on the GPU");
  for (const at::Tensor* t : {&out, &geom, &flip, &scale, &bias})
    TORCH_CHECK(t->device() == src.device(), op, ": tensors are on different devices");
  TORCH_CHECK(src.scalar_type() == at::kByte, op, ": src must be uint8, got ", src.scalar_type());
  TORCH_CHECK(src.dim() == 4 && src.size(3) == 3, op, ": src must be [N, Hs, Ws, 3] (3 channels last)");
  TORCH_CHECK(src.is_contiguous(), op, ": src must be contiguous");
  const int out_dtype = dtype_code(out);
  TORCH_CHECK(out.dim() == 4 && out.size(1) == 3 && (index || out.size(0) == src.size(0)), op,
              ": out must be [N, 3, Ho, Wo] with src's N");
  if (index) {
    TORCH_CHECK(index->is_cuda() && index->device() == src.device(), op, ": index must be on the store's GPU");
    TORCH_CHECK(index->scalar_type() == at::kInt && index->dim() == 1 && index->is_contiguous(), op,
                ": index must be a contiguous int32 [N], got ", index->scalar_type());
    TORCH_CHECK(index->size(0) == out.size(0), op, ": index has ", index->size(0), " entries, out ", out.size(0),
                " images");
    TORCH_CHECK(src.size(0) >= 1 && src.size(0) < (int64_t(1) << 31), op, ": the store must hold 1 <= P < 2^31 images");
  }
  const int64_t N = out.size(0), Hs = src.size(1), Ws = src.size(2), Ho = out.size(2), Wo = out.size(3);
  TORCH_CHECK(Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, op, ": empty image");
  const int64_t want[4] = {Ho * Wo * 3, 1, Wo * 3, 3};
  for (int d = 0; d < 4; ++d)
    TORCH_CHECK(out.size(d) == 1 || out.stride(d) == want[d], op,
                ": out must be channels-last memory (dense [N, Ho, Wo, 3]); stride ", out.stride(d), " of dim ", d,
                ", expected ", want[d]);
  TORCH_CHECK(geom.scalar_type() == at::kFloat && geom.dim() == 2 && geom.size(0) == N && geom.size(1) == 4 &&
                  geom.is_contiguous(),
              op, ": geom must be a contiguous fp32 [N, 4]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(geom.data_ptr()) % 16 == 0, op, ": geom must be 16-byte aligned");
  // a row's two x taps are read by one 8-byte load that is kept inside the tensor
  TORCH_CHECK(N == 0 || (index ? Hs * Ws : src.numel() / 3) >= 3, op,
              index ? ": an image must hold at least three pixels" : ": src must hold at least three pixels");
  TORCH_CHECK(flip.scalar_type() == at::kByte && flip.dim() == 1 && flip.size(0) == N && flip.is_contiguous(), op,
              ": flip must be a contiguous uint8 [N]");
  for (const at::Tensor* t : {&scale, &bias})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->numel() == 3 && t->is_contiguous(), op,
                ": scale and bias must be contiguous fp32 [3]");
  TORCH_CHECK(pad >= 0 && pad < (1 << 20), op, ": pad must be >= 0, got ", pad);
  TORCH_CHECK((index ? Hs * Ws * 3 : src.numel()) < (int64_t(1) << 31) && out.numel() < (int64_t(1) << 31), op,
              index ? ": an image and out must have fewer than 2^31 elements"
                    : ": src and out must have fewer than 2^31 elements");
  return AugmentDims{(int)N, (int)Hs, (int)Ws, (int)Ho, (int)Wo, out_dtype};
}

void augment_(at::Tensor src, at::Tensor out, at::Tensor geom, at::Tensor flip, at::Tensor scale, at::Tensor bias,
              int64_t pad) {
  const AugmentDims d = check_augment_args("augment_", src, out, geom, flip, scale, bias, pad);
  launch_augment(src.data_ptr<uint8_t>(), out.data_ptr(), d.dtype, geom.data_ptr<float>(), flip.data_ptr<uint8_t>(),
                 scale.data_ptr<float>(), bias.data_ptr<float>(), d.N, d.Hs, d.Ws, d.Ho, d.Wo, (int)pad,
                 current_stream(out));
}

// augment_ reading its batch in place from a resident store: image n is store row index[n] (dla_kernels.h). The
// values of index live on the device and are the caller's to keep in [0, P) (ops/augment.py checks a host index).
void augment_gather_(at::Tensor store, at::Tensor index, at::Tensor out, at::Tensor geom, at::Tensor flip,
                     at::Tensor scale, at::Tensor bias, int64_t pad) {
  const AugmentDims d = check_augment_args("augment_gather_", store, out, geom, flip, scale, bias, pad, &index);
  launch_augment_gather(store.data_ptr<uint8_t>(), store.size(0), index.data_ptr<int32_t>(), out.data_ptr(), d.dtype,
                        geom.data_ptr<float>(), flip.data_ptr<uint8_t>(), scale.data_ptr<float>(),
                        bias.data_ptr<float>(), d.N, d.Hs, d.Ws, d.Ho, d.Wo, (int)pad, current_stream(out));
}

// augment_ with Mixup / CutMix: per sample a partner image, a weight and a box on the output grid (dla_kernels.h).
// The values of partner, lam and box live on the device and are the caller's to keep in range (ops/augment.py
// checks host tensors); blend = false promises lam == 1 everywhere.
static void check_mix_args(const char* op, const at::Tensor& src, const AugmentDims& d, const at::Tensor& partner,
                           const at::Tensor& lam, const at::Tensor& box) {
  for (const at::Tensor* t : {&partner, &lam, &box})
    TORCH_CHECK(t->is_cuda() && t->device() == src.device(), op, ": partner, lam and box must be on src's GPU");
  TORCH_CHECK(partner.scalar_type() == at::kInt && partner.dim() == 1 && partner.size(0) == d.N &&
                  partner.is_contiguous(),
              op, ": partner must be a contiguous int32 [N]");
  TORCH_CHECK(lam.scalar_type() == at::kFloat && lam.dim() == 1 && lam.size(0) == d.N && lam.is_contiguous(), op,
              ": lam must be a contiguous fp32 [N]");
  TORCH_CHECK(box.scalar_type() == at::kInt && box.dim() == 2 && box.size(0) == d.N && box.size(1) == 4 &&
                  box.is_contiguous(),
              op, ": box must be a contiguous int32 [N, 4]");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(box.data_ptr()) % 16 == 0, op, ": box must be 16-byte aligned");
}

void augment_mix_(at::Tensor src, at::Tensor out, at::Tensor geom, at::Tensor flip, at::Tensor partner, at::Tensor lam,
                  at::Tensor box, at::Tensor scale, at::Tensor bias, int64_t pad, bool blend) {
  const AugmentDims d = check_augment_args("augment_mix_", src, out, geom, flip, scale, bias, pad);
  check_mix_args("augment_mix_", src, d, partner, lam, box);
  launch_augment_mix(src.data_ptr<uint8_t>(), out.data_ptr(), d.dtype, geom.data_ptr<float>(),
                     flip.data_ptr<uint8_t>(), partner.data_ptr<int32_t>(), lam.data_ptr<float>(),
                     box.data_ptr<int32_t>(), scale.data_ptr<float>(), bias.data_ptr<float>(), d.N, d.Hs, d.Ws, d.Ho,
                     d.Wo, (int)pad, blend, current_stream(out));
}

// augment_mix_ over a resident store: partner[n] is a position in the batch, whose image is row index[partner[n]].
void augment_mix_gather_(at::Tensor store, at::Tensor index, at::Tensor out, at::Tensor geom, at::Tensor flip,
                         at::Tensor partner, at::Tensor lam, at::Tensor box, at::Tensor scale, at::Tensor bias,
                         int64_t pad, bool blend) {
  const AugmentDims d = check_augment_args("augment_mix_gather_", store, out, geom, flip, scale, bias, pad, &index);
  check_mix_args("augment_mix_gather_", store, d, partner, lam, box);
  launch_augment_mix_gather(store.data_ptr<uint8_t>(), store.size(0), index.data_ptr<int32_t>(), out.data_ptr(),
                            d.dtype, geom.data_ptr<float>(), flip.data_ptr<uint8_t>(), partner.data_ptr<int32_t>(),
                            lam.data_ptr<float>(), box.data_ptr<int32_t>(), scale.data_ptr<float>(),
                            bias.data_ptr<float>(), d.N, d.Hs, d.Ws, d.Ho, d.Wo, (int)pad, blend, current_stream(out));
}

std::vector<at::Tensor> xent_fwd(at::Tensor logits, at::Tensor target) {
  check_dev(logits, "logits");
  check_dev(target, "target");
  TORCH_CHECK(logits.dim() == 2, "xent_fwd: logits must be [B, C]");
  TORCH_CHECK(target.scalar_type() == at::kLong && target.numel() == logits.size(0), "xent_fwd: bad target");
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  auto f32 = logits.options().dtype(at::kFloat);
  auto ws = at::empty({3 * (int64_t)B}, f32);
  auto loss = at::empty({2}, f32);
  launch_xent_fwd(logits.data_ptr(), target.data_ptr<int64_t>(), ws.data_ptr<float>(), loss.data_ptr<float>(), B, C,
                  dtype_code(logits), current_stream(logits));
  return {loss, ws};
}

at::Tensor xent_bwd(at::Tensor logits, at::Tensor target, at::Tensor ws, at::Tensor loss, at::Tensor gout) {
  check_dev(logits, "logits");
  auto d = at::empty_like(logits);
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  auto g = gout.to(at::kFloat).contiguous();
  launch_xent_bwd(logits.data_ptr(), target.data_ptr<int64_t>(), ws.data_ptr<float>(), loss.data_ptr<float>(),
                  g.data_ptr<float>(), d.data_ptr(), B, C, dtype_code(logits), current_stream(logits));
  return d;
}

// Counts are carried as floats: below 2^24 rows and classes every count and rank is exact.
constexpr int64_t kXentMaxDim = int64_t(1) << 24;

static void check_xent_args(const at::Tensor& logits, const at::Tensor& target, double eps, const char* op) {
  check_dev(logits, "logits");
  check_dev(target, "target");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), op, ": logits must be a contiguous [B, C]");
  TORCH_CHECK(target.scalar_type() == at::kLong && target.numel() == logits.size(0) && target.is_contiguous(), op,
              ": bad target");
  TORCH_CHECK(target.device() == logits.device(), op, ": logits and target are on different devices");
  TORCH_CHECK(logits.size(1) >= 1, op, ": no classes");
  TORCH_CHECK(logits.size(0) < kXentMaxDim && logits.size(1) < kXentMaxDim, op, ": B and C must be below 2^24");
  TORCH_CHECK(eps >= 0.0 && eps < 1.0, op, ": label smoothing must be in [0, 1), got ", eps);
}

std::vector<at::Tensor> xent_metrics_fwd(at::Tensor logits, at::Tensor target, double eps, int64_t k) {
  check_xent_args(logits, target, eps, "xent_metrics_fwd");
  TORCH_CHECK(k >= 1, "xent_metrics_fwd: k must be >= 1, got ", k);
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  auto f32 = logits.options().dtype(at::kFloat);
  auto ws = at::empty({4 * (int64_t)B + 1}, f32);
  auto stats = at::empty({4}, f32);
  launch_xent_metrics_fwd(logits.data_ptr(), target.data_ptr<int64_t>(), ws.data_ptr<float>(), stats.data_ptr<float>(),
                          B, C, (float)eps, (int)std::min(k, kXentMaxDim), dtype_code(logits), current_stream(logits));
  return {stats, ws};
}

// The forward's outputs as the backward wrappers get them back: nstats statistics, nstats / 2 + 2 workspace
// floats per row and the mean. Returns gout as a contiguous fp32 tensor.
static at::Tensor check_xent_bwd_args(const at::Tensor& ws, const at::Tensor& stats, const at::Tensor& gout, int B,
                                      int nstats, const char* op) {
  check_dev(ws, "ws");
  check_dev(stats, "stats");
  TORCH_CHECK(ws.scalar_type() == at::kFloat && ws.numel() == (nstats / 2 + 2) * (int64_t)B + 1, op,
              ": bad workspace");
  TORCH_CHECK(stats.scalar_type() == at::kFloat && stats.numel() == nstats, op, ": bad stats");
  TORCH_CHECK(gout.is_cuda() && gout.numel() == 1, op, ": gout must be one value on the GPU");
  return gout.to(at::kFloat).contiguous();
}

at::Tensor xent_smooth_bwd(at::Tensor logits, at::Tensor target, at::Tensor ws, at::Tensor stats, at::Tensor gout,
                           double eps) {
  check_xent_args(logits, target, eps, "xent_smooth_bwd");
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  auto g = check_xent_bwd_args(ws, stats, gout, B, 4, "xent_smooth_bwd");
  auto d = at::empty_like(logits);
  launch_xent_smooth_bwd(logits.data_ptr(), target.data_ptr<int64_t>(), ws.data_ptr<float>(), stats.data_ptr<float>(),
                         g.data_ptr<float>(), d.data_ptr(), B, C, (float)eps, dtype_code(logits),
                         current_stream(logits));
  return d;
}

static void check_xent_mix_args(const at::Tensor& logits, const at::Tensor& target_a, const at::Tensor& target_b,
                                const at::Tensor& lam, double eps, const char* op) {
  check_xent_args(logits, target_a, eps, op);
  check_xent_args(logits, target_b, eps, op);
  check_dev(lam, "lam");
  TORCH_CHECK(lam.scalar_type() == at::kFloat && lam.numel() == logits.size(0) && lam.is_contiguous(), op,
              ": lam must be a contiguous fp32 [B]");
  TORCH_CHECK(lam.device() == logits.device(), op, ": logits and lam are on different devices");
}

std::vector<at::Tensor> xent_mix_fwd(at::Tensor logits, at::Tensor target_a, at::Tensor target_b, at::Tensor lam,
                                     double eps) {
  check_xent_mix_args(logits, target_a, target_b, lam, eps, "xent_mix_fwd");
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  auto f32 = logits.options().dtype(at::kFloat);
  auto ws = at::empty({3 * (int64_t)B + 1}, f32);
  auto stats = at::empty({2}, f32);
  launch_xent_mix_fwd(logits.data_ptr(), target_a.data_ptr<int64_t>(), target_b.data_ptr<int64_t>(),
                      lam.data_ptr<float>(), ws.data_ptr<float>(), stats.data_ptr<float>(), B, C, (float)eps,
                      dtype_code(logits), current_stream(logits));
  return {stats, ws};
}

at::Tensor xent_mix_bwd(at::Tensor logits, at::Tensor target_a, at::Tensor target_b, at::Tensor lam, at::Tensor ws,
                        at::Tensor stats, at::Tensor gout, double eps) {
  check_xent_mix_args(logits, target_a, target_b, lam, eps, "xent_mix_bwd");
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  auto g = check_xent_bwd_args(ws, stats, gout, B, 2, "xent_mix_bwd");
  auto d = at::empty_like(logits);
  launch_xent_mix_bwd(logits.data_ptr(), target_a.data_ptr<int64_t>(), target_b.data_ptr<int64_t>(),
                      lam.data_ptr<float>(), ws.data_ptr<float>(), stats.data_ptr<float>(), g.data_ptr<float>(),
                      d.data_ptr(), B, C, (float)eps, dtype_code(logits), current_stream(logits));
  return d;
}

void bind_ops(pybind11::module& m) {
  pybind11::class_<SgdTable>(m, "SgdTable")
      .def(pybind11::init<std::vector<at::Tensor>, std::vector<at::Tensor>, std::vector<at::Tensor>,
                          std::vector<at::Tensor>>())
      .def("step", &SgdTable::step)
      .def("num_blocks", &SgdTable::num_blocks);
  pybind11::class_<PackTable>(m, "PackTable")
      .def(pybind11::init<std::vector<at::Tensor>, std::vector<int64_t>>())
      .def("pack", &PackTable::pack)
      .def("unpack", &PackTable::unpack)
      .def("total_numel", &PackTable::total_numel);
  m.def("reduce_sum_", &reduce_sum_, "dst = scale*([dst] + sum(srcs))");
  m.def("sgd_step_list", &sgd_step_list, "fused SGD over a by-value tensor list (<= 32 tensors per launch)");
  pybind11::class_<LarsPlan>(m, "LarsPlan")
      .def(pybind11::init<std::vector<int64_t>, std::vector<int64_t>, std::vector<bool>, std::vector<double>,
                          std::vector<double>, std::vector<double>, std::vector<double>, c10::optional<at::Tensor>,
                          at::Tensor>())
      .def("grad_norm", &LarsPlan::grad_norm)
      .def("local_lr", &LarsPlan::local_lr)
      .def("norms", &LarsPlan::norms)
      .def("last_launches", &LarsPlan::last_launches);
  m.def("lars_step_list", &lars_step_list,
        "fused LARS over by-value tensor lists: square sums, finalize (norms, clip, trust), update");
  pybind11::class_<AdamPlan>(m, "AdamPlan")
      .def(pybind11::init<bool, std::vector<int64_t>, std::vector<int64_t>, std::vector<bool>, std::vector<double>,
                          std::vector<double>, std::vector<double>, std::vector<double>, std::vector<at::Tensor>,
                          at::Tensor, at::Tensor>())
      .def("grad_norm", &AdamPlan::grad_norm)
      .def("alpha", &AdamPlan::alpha)
      .def("bias_corrections", &AdamPlan::bias_corrections)
      .def("norms", &AdamPlan::norms)
      .def("last_launches", &AdamPlan::last_launches);
  m.def("lamb_step_list", &adam_step_list<true>,
        "fused LAMB over by-value tensor lists: moments + square sums, finalize (trust, bias corrections, step "
        "counts), apply; with max_grad_norm > 0 a gradient square-sum pass and its finalize first");
  m.def("adamw_step_list", &adam_step_list<false>,
        "fused AdamW over by-value tensor lists: finalize (bias corrections, step counts), one update pass");
  m.def("lamb_ema_step_list", &adam_ema_step_list<true>, "lamb_step_list with the weight EMA in the apply launches");
  m.def("adamw_ema_step_list", &adam_ema_step_list<false>, "adamw_step_list with the weight EMA in the update launches");
  m.def("sgd_ema_step_list", &sgd_ema_step_list,
        "sgd_step_list with the weight EMA in the same launches: ema = fmaf(omd, p_new - ema, ema), omd on the device");
  m.def("lars_ema_step_list", &lars_ema_step_list, "lars_step_list with the weight EMA in the update launches");
  m.def("ema_update_list", &ema_update_list, "emas[i] = fmaf(omd, srcs[i] - emas[i], emas[i]) over fp32 tensor lists");
  m.def("ema_swap_list", &ema_swap_list,
        "exchange fp32 targets with their EMAs in place; shadows[i] (bf16 or None) = bf16(new target)",
        pybind11::arg("targets"), pybind11::arg("emas"),
        pybind11::arg("shadows") = std::vector<c10::optional<at::Tensor>>());
  m.def("multi_tensor_l2norm", &multi_tensor_l2norm, "(per-tensor, total) L2 norms of a tensor list times scale");
  m.def("pack_list", &pack_list, "gather tensors into a flat buffer at element offsets (by-value list launch)");
  m.def("scale_", &scale_, "t *= scale");
  m.def("uniform_", &uniform_, "Philox uniform fill (stream position offset [+ *step * per_step])",
        pybind11::arg("t"), pybind11::arg("seed"), pybind11::arg("offset"), pybind11::arg("lo"), pybind11::arg("hi"),
        pybind11::arg("step") = pybind11::none(), pybind11::arg("per_step") = 0);
  m.def("randint_", &randint_, "Philox integer fill in [0, high)", pybind11::arg("t"), pybind11::arg("high"),
        pybind11::arg("seed"), pybind11::arg("offset"), pybind11::arg("step") = pybind11::none(),
        pybind11::arg("per_step") = 0);
  m.def("augment_", &augment_,
        "uint8 [N,Hs,Ws,3] -> channels-last [N,3,Ho,Wo]: per-sample crop, bilinear resample, flip, normalise, cast",
        pybind11::arg("src"), pybind11::arg("out"), pybind11::arg("geom"), pybind11::arg("flip"),
        pybind11::arg("scale"), pybind11::arg("bias"), pybind11::arg("pad") = 0);
  m.def("augment_mix_", &augment_mix_,
        "augment_ with Mixup / CutMix: out = fmaf(w, A(n), (1 - w) * A(partner[n])), w = 0 inside box[n] else lam[n]; "
        "blend = false samples once per pixel and needs lam == 1",
        pybind11::arg("src"), pybind11::arg("out"), pybind11::arg("geom"), pybind11::arg("flip"),
        pybind11::arg("partner"), pybind11::arg("lam"), pybind11::arg("box"), pybind11::arg("scale"),
        pybind11::arg("bias"), pybind11::arg("pad") = 0, pybind11::arg("blend") = true);
  m.def("augment_gather_", &augment_gather_,
        "augment_ reading image n in place from row index[n] of a resident uint8 store [P,Hs,Ws,3] of any size",
        pybind11::arg("store"), pybind11::arg("index"), pybind11::arg("out"), pybind11::arg("geom"),
        pybind11::arg("flip"), pybind11::arg("scale"), pybind11::arg("bias"), pybind11::arg("pad") = 0);
  m.def("augment_mix_gather_", &augment_mix_gather_,
        "augment_mix_ over a resident store: image n is row index[n], its partner row index[partner[n]]",
        pybind11::arg("store"), pybind11::arg("index"), pybind11::arg("out"), pybind11::arg("geom"),
        pybind11::arg("flip"), pybind11::arg("partner"), pybind11::arg("lam"), pybind11::arg("box"),
        pybind11::arg("scale"), pybind11::arg("bias"), pybind11::arg("pad") = 0, pybind11::arg("blend") = true);
  m.def("xent_fwd", &xent_fwd, "fused log-softmax + NLL forward");
  m.def("xent_bwd", &xent_bwd, "fused log-softmax + NLL backward");
  m.def("xent_metrics_fwd", &xent_metrics_fwd,
        "label-smoothed cross-entropy forward: (stats[4] = loss sum, valid rows, top-1 correct, top-k correct; ws, whose "
        "last element is the mean loss)");
  m.def("xent_smooth_bwd", &xent_smooth_bwd, "label-smoothed cross-entropy backward");
  m.def("xent_mix_fwd", &xent_mix_fwd,
        "pair-target label-smoothed cross-entropy forward: (stats[2] = loss sum, valid rows; ws, whose last element is "
        "the mean loss)");
  m.def("xent_mix_bwd", &xent_mix_bwd, "pair-target label-smoothed cross-entropy backward");
}

}  // namespace dla
