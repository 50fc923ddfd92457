// Conjugate gradient as a workload: one schedule run is one CG iteration on A x = b.
//
// Not in the reference (its SpMV workload is the single product y = A x). An iteration is one
// SpMV, two global reductions and three vector updates; at 150,000 rows each kernel takes a few
// microseconds, so which ops are fused and which run side by side decides the iteration time.
//
// Scalars (rr = r . r, alpha, beta) are f64 values in device memory and every dot product is a
// slab of per-block partials that its consumer sums (kernels/cg_kernels.hip). Each scalar and
// each slab has exactly one writer op per form, and the graph's edges keep that writer from
// overlapping any reader:
//   plain: alpha <- cg_alpha, beta and rr <- cg_beta, pq slab <- dot_pq, rr slab <- dot_rr
//   fused: pq slab <- spmvdot, rr slab <- the r update, rr <- block 0 of the next iteration's
//          spmvdot (after the last reader of the old rr, the p update, and before the first
//          reader of the new one); alpha and beta live in registers only
//   sr:    the single-reduction (Chronopoulos-Gear) recurrence, two launches. gamma slab (the rr
//          slab's place) and delta slab (the pq slab's) <- spmvdot; gamma, alpha, beta <- block 0
//          of the update, which no block of that launch reads; gamma_prev, alpha_prev <- block 0
//          of the next iteration's spmvdot, which copies them from gamma and alpha (after their
//          last reader, the update, and before the next one). With nrhs = 2, 4 or 8 the same
//          two ops run the batched kernels on interleaved vectors: nrhs independent recurrences,
//          every slab and scalar an array of nrhs with the same writers. With tol > 0 the two
//          ops launch the stopping kernels: thresholds <- the host (reset, set_armed), done,
//          iters and all_done <- block 0 of the update, read by the next spmvdot (dStop_).
//          With precond jacobi the two ops launch the preconditioned pair: the same writers and
//          readers, and rho slab <- spmvdot, read by the stopping update; u <- the update (and
//          reset), read by the next spmvdot; dinv <- setup, read by the update
//          With refine_tol > 0 the same two ops with the same arguments. refine_step() is no op
//          of the graph: between two device synchronizes, on the null stream, it writes x64, r64,
//          its two slabs and the outer state (dRefine_, a buffer of its own), and x, s, r, p (u),
//          the inner threshold, done and the five scalars, as reset() writes them
#include "workloads.hpp"

#include "core/util.hpp"
#include "hip/hip_runtime.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <random>

namespace tz {

Json CgArgs::json() const {
  Json j;
  j["m"] = m;
  j["bw"] = bw;
  j["nnz"] = nnz;
  j["nnz_actual"] = nnz_actual;
  j["seed"] = int64_t(seed);
  j["matrix"] = matrix;
  j["form"] = form;
  j["lanes"] = lanes;
  j["rhs"] = rhs;
  j["nrhs"] = nrhs;
  j["rhs_first"] = rhs_first;
  j["tol"] = tol;
  j["precond"] = precond;
  j["diag_scale"] = diag_scale;
  j["refine_tol"] = refine_tol;
  j["rank"] = rank;
  j["size"] = size;
  return j;
}

namespace {

// the kernels' order (kern::sum_partials_f64): xor butterfly over each 64 partials, then the
// four groups in order
double sum_partials_host(const double *p, int np) {
  double total = 0.0;
  for (int w = 0; w < 4; ++w) {
    double v[64], t[64];
    for (int l = 0; l < 64; ++l) v[l] = w * 64 + l < np ? p[w * 64 + l] : 0.0;
    for (int off = 32; off > 0; off >>= 1) {
      for (int l = 0; l < 64; ++l) t[l] = v[l] + v[l ^ off];
      std::copy(t, t + 64, v);
    }
    total = w == 0 ? v[0] : total + v[0];
  }
  return total;
}

using Body = void (ConjugateGradient::*)(void *) const;

class CgOp : public GpuOp {
public:
  CgOp(std::shared_ptr<const ConjugateGradient> c, std::string name, std::string kind, Body body,
       double latencyUs, double bytes, double rate)
      : c_(std::move(c)), name_(std::move(name)), kind_(std::move(kind)), body_(body), lat_(latencyUs),
        bytes_(bytes), rate_(rate) {}
  std::string name() const override { return name_; }
  std::string kind() const override { return kind_; }
  double bytes() const override { return bytes_; }
  // a launch plus its bytes at `rate_` bytes per microsecond (gathers run below streaming rate)
  double cost_us() const override { return lat_ + bytes_ / rate_; }
  std::vector<Traffic> traffic() const override {
    if (bytes_ <= 0) return {};
    return {{"hbm", "kernel", bytes_}};
  }
  double latency_us() const override { return lat_; }
  void launch(void *st, Executor &) const override { ((*c_).*body_)(st); }

private:
  std::shared_ptr<const ConjugateGradient> c_;
  std::string name_, kind_;
  Body body_;
  double lat_, bytes_, rate_;
};

} // namespace

ConjugateGradient::ConjugateGradient(CgArgs a) : a_(std::move(a)) {
  TZ_CHECK(a_.size == 1 && a_.rank == 0,
           "the conjugate-gradient workload runs on one rank only (got rank " << a_.rank << " of " << a_.size
               << "): several ranks need a halo of p and an allreduce per dot product");
  TZ_CHECK(a_.form == "choice" || a_.form == "plain" || a_.form == "fused" || a_.form == "sr" || a_.form == "all",
           "CG form must be choice, plain, fused, sr or all (got " << a_.form << ")");
  TZ_CHECK(a_.rhs == "random" || a_.rhs == "zero", "CG rhs must be random or zero (got " << a_.rhs << ")");
  TZ_CHECK(a_.nrhs == 1 || a_.nrhs == 2 || a_.nrhs == 4 || a_.nrhs == 8,
           "CG nrhs must be 1, 2, 4 or 8 right-hand sides (got " << a_.nrhs << "): a row of the batch is one "
               << "16-byte-aligned run inside a 128-byte line");
  TZ_CHECK(a_.nrhs == 1 || a_.form == "sr",
           "CG with nrhs > 1 needs form sr: only the single-reduction form has batched kernels (got nrhs "
               << a_.nrhs << " with form " << a_.form << ")");
  TZ_CHECK(a_.rhs_first >= 0, "CG rhs_first must not be negative (got " << a_.rhs_first << ")");
  TZ_CHECK(std::isfinite(a_.tol) && a_.tol >= 0, "CG tol must be finite and not negative (got " << a_.tol << ")");
  TZ_CHECK(std::isfinite(a_.refine_tol) && a_.refine_tol >= 0,
           "CG refine_tol must be finite and not negative (got " << a_.refine_tol << ")");
  if (a_.refine_tol > 0) {
    TZ_CHECK(a_.form == "sr", "CG with refine_tol > 0 needs form sr: the refinement step restarts the "
                                  << "single-reduction recurrence (got refine_tol " << a_.refine_tol << " with form "
                                  << a_.form << ")");
    TZ_CHECK(a_.nrhs == 1, "CG with refine_tol > 0 needs nrhs 1: batched refinement is not built (got nrhs "
                               << a_.nrhs << ")");
    TZ_CHECK(a_.tol > 0, "CG with refine_tol > 0 needs tol > 0: tol is the inner solve's relative tolerance, "
                             << "and without it the f32 solve never stops (got tol 0)");
    TZ_CHECK(a_.refine_tol < a_.tol, "CG refine_tol must be below tol: the inner f32 solve to tol already reaches "
                                         << "tol, refinement is for what lies beyond it (got refine_tol "
                                         << a_.refine_tol << " with tol " << a_.tol << ")");
  }
  TZ_CHECK(a_.tol == 0 || a_.form == "sr",
           "CG with tol > 0 needs form sr: only the single-reduction form has kernels that test convergence "
               << "on the device (got tol " << a_.tol << " with form " << a_.form << ")");
  TZ_CHECK(a_.precond == "none" || a_.precond == "jacobi",
           "CG precond must be none or jacobi (got " << a_.precond << ")");
  TZ_CHECK(a_.precond == "none" || (a_.form == "sr" && a_.nrhs == 1),
           "CG with precond " << a_.precond << " needs form sr and nrhs 1: only the single-reduction form for "
               << "one right-hand side has preconditioned kernels (got form " << a_.form << " with nrhs "
               << a_.nrhs << ")");
  TZ_CHECK(a_.diag_scale >= 0 && a_.diag_scale <= 8, "CG diag_scale must be 0..8 (got " << a_.diag_scale << ")");
  if (!a_.matrix.empty()) {
    A_ = read_matrix_market(a_.matrix);
    TZ_CHECK(A_.rows == A_.cols, a_.matrix << ": CG needs a square matrix, got " << A_.rows << " x " << A_.cols);
    // symmetric: every entry (r, c, v) has its mirror (c, r, v)
    for (int64_t r = 0; r < A_.rows; ++r)
      for (int32_t j = A_.rowPtr[size_t(r)]; j < A_.rowPtr[size_t(r + 1)]; ++j) {
        const int32_t c = A_.colInd[size_t(j)];
        const auto b0 = A_.colInd.begin() + A_.rowPtr[size_t(c)], b1 = A_.colInd.begin() + A_.rowPtr[size_t(c) + 1];
        const auto it = std::lower_bound(b0, b1, int32_t(r));
        TZ_CHECK(it != b1 && *it == int32_t(r) && A_.val[size_t(it - A_.colInd.begin())] == A_.val[size_t(j)],
                 a_.matrix << ": not symmetric at (" << r + 1 << ", " << c + 1 << "): CG needs a symmetric "
                           << "positive definite matrix");
      }
    a_.m = A_.rows;
    a_.bw = 0;
    a_.nnz = A_.nnz();
  } else {
    TZ_CHECK(a_.m > 0, "CG needs at least one row");
    if (a_.bw <= 0) a_.bw = a_.m;
    if (a_.nnz <= 0) a_.nnz = 5 * a_.m;
    A_ = spd_band_matrix(a_.m, a_.bw, a_.nnz, a_.seed);
  }
  TZ_CHECK(A_.rows < (int64_t(1) << 31) / 4, "CG: too many rows");
  a_.nnz_actual = A_.nnz();
  b_.assign(size_t(a_.nrhs), std::vector<float>(size_t(A_.rows), 0.f));
  if (a_.rhs == "random") {
    for (int c = 0; c < a_.nrhs; ++c) {
      // 24 random bits per entry: k / 2^23 - 1 is exact in f32 and lies in [-1, 1). Right-hand
      // side number j of the sequence reseeds the generator (j = 0: the single solve's b).
      const uint64_t j = uint64_t(a_.rhs_first) + uint64_t(c);
      std::mt19937_64 rng((a_.seed ^ 0xC6A4A7935BD1E995ull) + j * 0x9E3779B97F4A7C15ull);
      for (float &v : b_[size_t(c)]) v = float(int64_t(rng() >> 40)) / 8388608.f - 1.f;
    }
  }
  // the change of units: powers of two, so every product below is exact
  scale_.assign(size_t(A_.rows), 1.f);
  if (a_.diag_scale > 0) {
    std::mt19937_64 rng(a_.seed ^ 0xD1B54A32D192ED03ull);
    const uint64_t span = 2 * uint64_t(a_.diag_scale) + 1;
    for (float &s : scale_) s = std::ldexp(1.f, int(rng() % span) - a_.diag_scale);
    for (int64_t r = 0; r < A_.rows; ++r)
      for (int32_t j = A_.rowPtr[size_t(r)]; j < A_.rowPtr[size_t(r + 1)]; ++j)
        A_.val[size_t(j)] *= scale_[size_t(r)] * scale_[size_t(A_.colInd[size_t(j)])];
    for (std::vector<float> &bc : b_)
      for (size_t i = 0; i < bc.size(); ++i) bc[i] *= scale_[i];
  }
  if (jacobi()) {
    dinv_.resize(size_t(A_.rows));
    for (int64_t r = 0; r < A_.rows; ++r) {
      const auto b0 = A_.colInd.begin() + A_.rowPtr[size_t(r)], b1 = A_.colInd.begin() + A_.rowPtr[size_t(r + 1)];
      const auto it = std::find(b0, b1, int32_t(r));
      TZ_CHECK(it != b1, "CG precond jacobi: row " << r + 1 << " has no diagonal entry");
      const float d = A_.val[size_t(it - A_.colInd.begin())];
      TZ_CHECK(std::isfinite(d) && d > 0,
               "CG precond jacobi: row " << r + 1 << " has the diagonal entry " << d << ", which is not positive "
                                         << "and finite");
      dinv_[size_t(r)] = 1.0f / d;
    }
    // u = dinv o b, each product rounded to f32 once (a product alone: nothing to contract with)
    u0_.resize(dinv_.size());
    for (size_t i = 0; i < u0_.size(); ++i) u0_[i] = dinv_[i] * b_[0][i];
  }
  // the armed thresholds tol^2 * sum_i b[i]^2: the sum in f64 in index order, then one product
  // with tol * tol
  for (int c = 0; c < a_.nrhs && a_.tol > 0; ++c) {
    double bb = 0;
    for (float v : b_[size_t(c)]) bb += double(v) * double(v);
    thresh_.push_back(a_.tol * a_.tol * bb);
    if (refining()) outerThresh_ = a_.refine_tol * a_.refine_tol * bb; // nrhs = 1: the same b . b
  }
  const int W = a_.lanes - kern::kSpmvIlp;
  TZ_CHECK(a_.lanes == -1 || a_.lanes == 0 || W == 1 || W == 2 || W == 4 ||
               (a_.lanes > 0 && a_.lanes <= 64 && (a_.lanes & (a_.lanes - 1)) == 0),
           "CG lanes: a kern::csr_spmv variant (got " << a_.lanes << ")");
}

void ConjugateGradient::setup() {
  if (ready()) return;
  if (a_.device >= 0) TZ_HIP(hipSetDevice(a_.device));
  auto up = [](DeviceBuffer &d, const void *p, size_t bytes) {
    d = DeviceBuffer(std::max<size_t>(bytes, 16));
    d.upload(p, bytes);
  };
  up(dRow_, A_.rowPtr.data(), A_.rowPtr.size() * 4);
  up(dCol_, A_.colInd.data(), A_.colInd.size() * 4);
  up(dVal_, A_.val.data(), A_.val.size() * 4);
  // the right-hand sides as the kernels hold every vector: element (i, j) at i * nrhs + j
  const size_t k = size_t(a_.nrhs);
  std::vector<float> bi(size_t(rows()) * k);
  for (size_t c = 0; c < k; ++c)
    for (size_t i = 0; i < size_t(rows()); ++i) bi[i * k + c] = b_[c][i];
  up(dB_, bi.data(), bi.size() * 4);
  const size_t vb = std::max<size_t>(size_t(rows()) * k * 4, 16);
  dR_ = DeviceBuffer(vb);
  dP_ = DeviceBuffer(vb);
  dQ_ = DeviceBuffer(vb);
  dS_ = DeviceBuffer(vb);
  dW_ = DeviceBuffer(vb);
  dScal_ = DeviceBuffer((4 * size_t(kern::kCgMaxPartials) + 8) * sizeof(double));
  if (jacobi()) {
    up(dDinv_, dinv_.data(), dinv_.size() * 4);
    dU_ = DeviceBuffer(vb);
  }
  if (a_.nrhs > 1) dBatch_ = DeviceBuffer((2 * size_t(kern::kCgMaxPartials) + 5) * k * sizeof(double));
  if (a_.tol > 0) dStop_ = DeviceBuffer(size_t(a_.nrhs) * 20 + 4);
  if (refining()) {
    dX64_ = DeviceBuffer(std::max<size_t>(size_t(rows()) * sizeof(double), 16));
    dR64_ = DeviceBuffer(dX64_.bytes());
    dRefine_ = DeviceBuffer((2 * size_t(kern::kCgMaxPartials) + 4) * sizeof(double));
  }
  dX_ = DeviceBuffer(vb);
  reset();
}

void ConjugateGradient::reset() {
  TZ_CHECK(ready(), "CG not set up");
  // synchronous: schedules run on non-blocking streams that do not order after the null stream
  TZ_HIP(hipDeviceSynchronize());
  const size_t vb = size_t(rows()) * size_t(a_.nrhs) * 4;
  TZ_HIP(hipMemset(dX_.get(), 0, dX_.bytes()));
  TZ_HIP(hipMemset(dQ_.get(), 0, dQ_.bytes()));
  TZ_HIP(hipMemset(dS_.get(), 0, dS_.bytes()));
  TZ_HIP(hipMemset(dW_.get(), 0, dW_.bytes()));
  TZ_HIP(hipMemset(dScal_.get(), 0, dScal_.bytes()));
  TZ_HIP(hipMemcpy(dR_.get(), dB_.get(), vb, hipMemcpyDeviceToDevice));
  TZ_HIP(hipMemcpy(dP_.get(), dB_.get(), vb, hipMemcpyDeviceToDevice));
  if (jacobi()) dU_.upload(u0_.data(), u0_.size() * 4);
  if (a_.tol > 0) { // iters, done and all_done 0; armed
    TZ_HIP(hipMemset(dStop_.get(), 0, dStop_.bytes()));
    armed_ = true;
    upload_thresholds();
  }
  if (refining()) { // x64 = r64 = 0, both slabs, the step count and the flag 0; the outer threshold
    TZ_HIP(hipMemset(dX64_.get(), 0, dX64_.bytes()));
    TZ_HIP(hipMemset(dR64_.get(), 0, dR64_.bytes()));
    TZ_HIP(hipMemset(dRefine_.get(), 0, dRefine_.bytes()));
    TZ_HIP(hipMemcpy(rfThresh_(), &outerThresh_, sizeof(double), hipMemcpyHostToDevice));
    stepped_ = false;
  }
  if (a_.nrhs > 1) { // the batched form keeps no rr: every scalar array starts at 0
    TZ_HIP(hipMemset(dBatch_.get(), 0, dBatch_.bytes()));
    TZ_HIP(hipDeviceSynchronize());
    return;
  }
  kern::dot_partials_f32(rows(), dR_.as<float>(), dR_.as<float>(), rrp_(), nullptr);
  kern::sum_partials_f64(rrp_(), np_vec(), rr_(), nullptr);
  TZ_HIP(hipDeviceSynchronize());
}

void ConjugateGradient::upload_thresholds() const {
  const std::vector<double> off(thresh_.size(), -1.0);
  TZ_HIP(hipMemcpy(stThresh_(), (armed_ ? thresh_ : off).data(), thresh_.size() * sizeof(double),
                   hipMemcpyHostToDevice));
}

void ConjugateGradient::set_armed(bool armed) {
  TZ_CHECK(ready(), "CG not set up");
  TZ_CHECK(a_.tol > 0, "CG set_armed: this workload was built with tol = 0 and has no stopping test");
  TZ_CHECK(!stepped_, "CG set_armed: a refinement step was taken since the last reset(), and the inner threshold "
                          << "is the device's now; reset() first");
  TZ_HIP(hipDeviceSynchronize());
  armed_ = armed;
  upload_thresholds();
  if (!armed) TZ_HIP(hipMemset(stDone_(), 0, size_t(a_.nrhs + 1) * sizeof(int))); // done and all_done
  TZ_HIP(hipDeviceSynchronize());
}

int64_t ConjugateGradient::iterations(int col) const {
  TZ_CHECK(ready(), "CG not set up");
  TZ_CHECK(a_.tol > 0, "CG iterations: this workload was built with tol = 0 and counts nothing");
  checked(col);
  TZ_HIP(hipDeviceSynchronize());
  int64_t v = 0;
  TZ_HIP(hipMemcpy(&v, stIters_() + col, sizeof v, hipMemcpyDeviceToHost));
  return v;
}

bool ConjugateGradient::converged(int col) const {
  TZ_CHECK(ready(), "CG not set up");
  TZ_CHECK(a_.tol > 0, "CG converged: this workload was built with tol = 0 and tests nothing");
  checked(col);
  TZ_HIP(hipDeviceSynchronize());
  int v = 0;
  TZ_HIP(hipMemcpy(&v, stDone_() + col, sizeof v, hipMemcpyDeviceToHost));
  return v != 0;
}

double ConjugateGradient::threshold(int col) const {
  TZ_CHECK(a_.tol > 0, "CG threshold: this workload was built with tol = 0");
  if (ready()) TZ_HIP(hipDeviceSynchronize());
  return thresh_[size_t(checked(col))];
}

// ------------------------------------------------------------------ iterative refinement

void ConjugateGradient::check_refining(const char *what) const {
  TZ_CHECK(refining(), "CG " << what << ": this workload was built with refine_tol = 0 and keeps no f64 state");
  TZ_CHECK(ready(), "CG not set up");
}

void ConjugateGradient::refine_step() {
  check_refining("refine_step");
  TZ_CHECK(armed_, "CG refine_step: the workload is disarmed (set_armed(false)); a step restarts the inner solve "
                       << "with a threshold of its own, so reset() first");
  // synchronous like reset(): schedules run on non-blocking streams that the null stream does not order with
  TZ_HIP(hipDeviceSynchronize());
  stepped_ = true;
  const kern::SrState st = sr_state();
  kern::cg_refine_accumulate(rows(), dX_.as<float>(), dS_.as<float>(), dX64_.as<double>(), rfDone_(), nullptr);
  kern::cg_refine_residual(int(rows()), dRow_.as<int32_t>(), dCol_.as<int32_t>(), dVal_.as<float>(),
                           dB_.as<float>(), dX64_.as<double>(), jacobi() ? dDinv_.as<float>() : nullptr,
                           dR64_.as<double>(), dR_.as<float>(), dP_.as<float>(),
                           jacobi() ? dU_.as<float>() : nullptr, rfP64_(), rfP32_(), rfDone_(), nullptr);
  kern::RefineOuter o;
  o.thresh = rfThresh_(), o.done = rfDone_(), o.steps = rfSteps_(), o.rr64 = rfRr64_();
  kern::cg_refine_decide(rfP64_(), rfP32_(), kern::cg_refine_partial_count(int(rows())), a_.tol * a_.tol,
                         stThresh_(), st.done, st.gamma, st.alpha, st.beta, st.gamma_prev, st.alpha_prev, o, nullptr);
  TZ_HIP(hipDeviceSynchronize());
}

std::vector<double> ConjugateGradient::down64(const DeviceBuffer &d) const {
  TZ_HIP(hipDeviceSynchronize());
  std::vector<double> v(static_cast<size_t>(rows()));
  d.download(v.data(), v.size() * sizeof(double));
  return v;
}

std::vector<double> ConjugateGradient::x64() const {
  check_refining("x64");
  return down64(dX64_);
}

std::vector<double> ConjugateGradient::r64() const {
  check_refining("r64");
  return down64(dR64_);
}

namespace {
template <typename T> T peek(const T *dev) {
  TZ_HIP(hipDeviceSynchronize());
  T v{};
  TZ_HIP(hipMemcpy(&v, dev, sizeof v, hipMemcpyDeviceToHost));
  return v;
}
} // namespace

int64_t ConjugateGradient::outer_steps() const {
  check_refining("outer_steps");
  return peek(rfSteps_());
}

bool ConjugateGradient::refined() const {
  check_refining("refined");
  return peek(rfDone_()) != 0;
}

double ConjugateGradient::inner_threshold() const {
  check_refining("inner_threshold");
  return peek(stThresh_());
}

double ConjugateGradient::rr64() const {
  check_refining("rr64");
  return peek(rfRr64_());
}

double ConjugateGradient::outer_threshold() const {
  TZ_CHECK(refining(), "CG outer_threshold: this workload was built with refine_tol = 0");
  return outerThresh_;
}

double ConjugateGradient::residual64() const {
  const std::vector<double> xd = this->x64();
  const std::vector<float> &bc = this->b(0);
  double res = 0, bb = 0;
  for (size_t i = 0; i < size_t(rows()); ++i) {
    double s = 0;
    for (int32_t j = A_.rowPtr[i]; j < A_.rowPtr[i + 1]; ++j)
      s += double(A_.val[size_t(j)]) * xd[size_t(A_.colInd[size_t(j)])];
    const double d = double(bc[i]) - s;
    res += d * d;
    bb += double(bc[i]) * double(bc[i]);
  }
  return bb > 0 ? std::sqrt(res / bb) : std::sqrt(res);
}

int ConjugateGradient::checked(int col) const {
  TZ_CHECK(col >= 0 && col < a_.nrhs, "CG column " << col << " out of range: " << a_.nrhs << " right-hand side(s)");
  return col;
}

std::vector<float> ConjugateGradient::down(const DeviceBuffer &d, int col) const {
  TZ_CHECK(ready(), "CG not set up");
  const size_t k = size_t(a_.nrhs), c = size_t(checked(col));
  TZ_HIP(hipDeviceSynchronize());
  std::vector<float> all(static_cast<size_t>(rows()) * k);
  d.download(all.data(), all.size() * 4);
  if (k == 1) return all;
  std::vector<float> v(static_cast<size_t>(rows()));
  for (size_t i = 0; i < v.size(); ++i) v[i] = all[i * k + c];
  return v;
}

std::vector<float> ConjugateGradient::u(int col) const {
  TZ_CHECK(jacobi(), "CG u: this workload was built with precond none and keeps no u");
  return down(dU_, col);
}

const std::vector<float> &ConjugateGradient::dinv() const {
  TZ_CHECK(jacobi(), "CG dinv: this workload was built with precond none");
  return dinv_;
}

double ConjugateGradient::rr(int col) const {
  TZ_CHECK(ready(), "CG not set up");
  checked(col);
  TZ_HIP(hipDeviceSynchronize());
  // from r itself: the single-reduction form's slabs hold the previous r's products. The layout
  // is dot_rr's and the fused r update's, so for those forms these are the bits of the rr slab.
  if (a_.nrhs > 1) { // a contiguous copy of the column: the layout, hence the bits, of a single solve
    const std::vector<float> rc = r(col);
    DeviceBuffer tmp(std::max<size_t>(rc.size() * 4, 16));
    tmp.upload(rc.data(), rc.size() * 4);
    kern::dot_partials_f32(rows(), tmp.as<float>(), tmp.as<float>(), scratch_(), nullptr);
    TZ_HIP(hipDeviceSynchronize());
  } else {
    kern::dot_partials_f32(rows(), dR_.as<float>(), dR_.as<float>(), scratch_(), nullptr);
    TZ_HIP(hipDeviceSynchronize());
  }
  std::vector<double> part(static_cast<size_t>(kern::kCgMaxPartials), 0.0);
  TZ_HIP(hipMemcpy(part.data(), scratch_(), size_t(np_vec()) * sizeof(double), hipMemcpyDeviceToHost));
  return sum_partials_host(part.data(), np_vec());
}

double ConjugateGradient::residual(int col) const {
  const std::vector<float> xd = this->x(col);
  const std::vector<float> &bc = this->b(col);
  double res = 0, bb = 0;
  for (size_t i = 0; i < size_t(rows()); ++i) {
    double s = 0;
    for (int32_t j = A_.rowPtr[i]; j < A_.rowPtr[i + 1]; ++j)
      s += double(A_.val[size_t(j)]) * double(xd[size_t(A_.colInd[size_t(j)])]);
    const double d = double(bc[i]) - s;
    res += d * d;
    bb += double(bc[i]) * double(bc[i]);
  }
  return bb > 0 ? std::sqrt(res / bb) : std::sqrt(res);
}

double ConjugateGradient::check(int k, int col) const {
  const size_t n = size_t(rows());
  const std::vector<float> &bc = this->b(col);
  // z = M^-1 r with M = diag(A) as the device holds it (dinv), or M = I: rr is r . z throughout
  const bool pc = jacobi();
  auto z = [&](size_t i, double ri) { return pc ? double(dinv_[i]) * ri : ri; };
  std::vector<double> x(n, 0.0), r(bc.begin(), bc.end()), p(n), q(n);
  double rr = 0;
  for (size_t i = 0; i < n; ++i) {
    p[i] = z(i, r[i]);
    rr += r[i] * p[i];
  }
  for (int it = 0; it < k; ++it) {
    double pq = 0;
    for (size_t i = 0; i < n; ++i) {
      double s = 0;
      for (int32_t j = A_.rowPtr[i]; j < A_.rowPtr[i + 1]; ++j)
        s += double(A_.val[size_t(j)]) * p[size_t(A_.colInd[size_t(j)])];
      q[i] = s;
      pq += p[i] * s;
    }
    const double alpha = pq != 0.0 ? rr / pq : 0.0;
    double rrNew = 0;
    for (size_t i = 0; i < n; ++i) {
      x[i] += alpha * p[i];
      r[i] -= alpha * q[i];
      rrNew += r[i] * z(i, r[i]);
    }
    const double beta = rr != 0.0 ? rrNew / rr : 0.0;
    rr = rrNew;
    for (size_t i = 0; i < n; ++i) p[i] = z(i, r[i]) + beta * p[i];
  }
  const std::vector<float> xd = this->x(col);
  double err = 0, scale = 0;
  for (size_t i = 0; i < n; ++i) {
    // (std::max(err, NaN) is err: a NaN would pass as no error at all)
    if (!std::isfinite(xd[i])) return std::numeric_limits<double>::infinity();
    err = std::max(err, std::abs(double(xd[i]) - x[i]));
    scale = std::max(scale, std::abs(x[i]));
  }
  return scale > 0 ? err / scale : err;
}

// ------------------------------------------------------------------ op bodies

void ConjugateGradient::spmv(void *s) const {
  kern::csr_spmv(int(rows()), dRow_.as<int32_t>(), dCol_.as<int32_t>(), dVal_.as<float>(), dP_.as<float>(),
                 dQ_.as<float>(), a_.lanes, false, s);
}
void ConjugateGradient::dot_pq(void *s) const {
  kern::dot_partials_f32(rows(), dP_.as<float>(), dQ_.as<float>(), pq_(), s);
}
void ConjugateGradient::alpha(void *s) const { kern::cg_alpha(pq_(), np_vec(), rr_(), alpha_(), s); }
void ConjugateGradient::update_x(void *s) const {
  kern::axpy_dev_f32(rows(), alpha_(), +1, dP_.as<float>(), dX_.as<float>(), s);
}
void ConjugateGradient::update_r(void *s) const {
  kern::axpy_dev_f32(rows(), alpha_(), -1, dQ_.as<float>(), dR_.as<float>(), s);
}
void ConjugateGradient::dot_rr(void *s) const {
  kern::dot_partials_f32(rows(), dR_.as<float>(), dR_.as<float>(), rrp_(), s);
}
void ConjugateGradient::beta(void *s) const { kern::cg_beta(rrp_(), np_vec(), rr_(), beta_(), s); }
void ConjugateGradient::update_p(void *s) const {
  kern::xpay_dev_f32(rows(), beta_(), dR_.as<float>(), dP_.as<float>(), s);
}
void ConjugateGradient::fused_spmv_dot(void *s) const {
  kern::csr_spmv_dot(int(rows()), dRow_.as<int32_t>(), dCol_.as<int32_t>(), dVal_.as<float>(), dP_.as<float>(),
                     dQ_.as<float>(), kFusedLanes, pq_(), rrp_(), np_vec(), rr_(), s);
}
void ConjugateGradient::fused_x(void *s) const {
  kern::cg_fused_x(rows(), pq_(), np_spmv(), rr_(), dP_.as<float>(), dX_.as<float>(), s);
}
void ConjugateGradient::fused_r(void *s) const {
  kern::cg_fused_r(rows(), pq_(), np_spmv(), rr_(), dQ_.as<float>(), dR_.as<float>(), rrp_(), s);
}
void ConjugateGradient::fused_p(void *s) const {
  kern::cg_fused_p(rows(), rrp_(), np_vec(), rr_(), dR_.as<float>(), dP_.as<float>(), s);
}

// dScal_'s layout for one right-hand side, dBatch_'s for several, and dStop_ with tol > 0
kern::SrState ConjugateGradient::sr_state() const {
  kern::SrState st;
  st.k = a_.nrhs;
  if (a_.nrhs > 1) {
    st.partials_gamma = bGamma_(), st.partials_delta = bDelta_();
    st.gamma = bScal_(0), st.alpha = bScal_(1), st.beta = bScal_(2), st.gamma_prev = bScal_(3), st.alpha_prev = bScal_(4);
  } else {
    st.partials_gamma = rrp_(), st.partials_delta = pq_();
    st.gamma = srGamma_(), st.alpha = srAlpha_(), st.beta = srBeta_();
    st.gamma_prev = srGammaPrev_(), st.alpha_prev = srAlphaPrev_();
  }
  if (a_.tol > 0) st.thresh = stThresh_(), st.done = stDone_(), st.iters = stIters_(), st.all_done = stAllDone_();
  if (jacobi()) st.partials_rho = rho_();
  return st;
}
void ConjugateGradient::pcg_spmv_dot(void *s) const {
  kern::sr_pcg_spmv_dot3(a_.tol > 0, int(rows()), dRow_.as<int32_t>(), dCol_.as<int32_t>(), dVal_.as<float>(),
                         dR_.as<float>(), dU_.as<float>(), dW_.as<float>(), kFusedLanes, sr_state(), s);
}
void ConjugateGradient::pcg_update(void *s) const {
  kern::sr_pcg_update(a_.tol > 0, rows(), np_spmv(), dW_.as<float>(), dDinv_.as<float>(), dR_.as<float>(),
                      dP_.as<float>(), dS_.as<float>(), dX_.as<float>(), dU_.as<float>(), sr_state(), s);
}
void ConjugateGradient::sr_spmv_dot(void *s) const {
  kern::sr_spmv_dot2(a_.nrhs > 1, a_.tol > 0, int(rows()), dRow_.as<int32_t>(), dCol_.as<int32_t>(),
                     dVal_.as<float>(), dR_.as<float>(), dW_.as<float>(), kFusedLanes, sr_state(), s);
}
void ConjugateGradient::sr_update(void *s) const {
  kern::sr_update(a_.nrhs > 1, a_.tol > 0, rows(), np_spmv(), dW_.as<float>(), dR_.as<float>(), dP_.as<float>(),
                  dS_.as<float>(), dX_.as<float>(), sr_state(), s);
}

// ------------------------------------------------------------------ graph

std::shared_ptr<Graph> ConjugateGradient::sr_graph() const {
  auto self = shared_from_this();
  const std::string p = a_.prefix + "s_";
  // cost model as in form_graph: the SpMV with two dots is the fused form's, the update one
  // launch with a two-slab prologue over 36 bytes per row (reads w, r, p, s, x; writes r, p, s, x).
  // With k right-hand sides the matrix (8 bytes per entry) is streamed once and every gather and
  // every vector is k times as wide; k = 1 gives spmv_bytes().
  const double k = double(a_.nrhs), nnz = double(A_.nnz()), n = double(rows());
  auto sd = std::make_shared<CgOp>(self, p + "spmvdot", "CgSpmvDot2", &ConjugateGradient::sr_spmv_dot, 4.5,
                                   8.0 * nnz + 4.0 * nnz * k + 8.0 * n * k, 3.0e6);
  auto up = std::make_shared<CgOp>(self, p + "update", "CgSrUpdate", &ConjugateGradient::sr_update, 3.5,
                                   36.0 * n * k, 4.0e6);
  if (jacobi()) {
    // the preconditioned pair, one right-hand side: the SpMV gathers u, reads r and u per row (8
    // bytes) and writes w; the update reads w, dinv, r, p, s, x and writes p, s, x, r, u (44 bytes
    // per row: the old u is recomputed, not read)
    sd = std::make_shared<CgOp>(self, p + "spmvdot", "CgPcgSpmvDot3", &ConjugateGradient::pcg_spmv_dot, 4.5,
                                12.0 * nnz + 12.0 * n, 3.0e6);
    up = std::make_shared<CgOp>(self, p + "update", "CgPcgUpdate", &ConjugateGradient::pcg_update, 3.5, 44.0 * n,
                                4.0e6);
  }
  auto g = std::make_shared<Graph>();
  g->start_then(sd);
  g->then(sd, up); // w, the slabs, gamma_prev and alpha_prev
  g->then_finish(up);
  return g;
}

std::shared_ptr<Graph> ConjugateGradient::form_graph(bool fused) const {
  auto self = shared_from_this();
  const std::string p = a_.prefix + (fused ? "f_" : "");
  const double n = double(rows());
  // cost model: a launch of ~3 us plus the bytes at 4e6 bytes / us (the SpMV workload's
  // VectorAdd), the SpMV's gathers at 3e6; a prologue that sums a slab adds a fraction of a us
  auto op = [&](const char *name, const char *kind, Body body, double lat, double bytes, double rate = 4.0e6) {
    return std::make_shared<CgOp>(self, p + name, kind, body, lat, bytes, rate);
  };
  auto g = std::make_shared<Graph>();
  if (fused) {
    auto sd = op("spmvdot", "CgSpmvDot", &ConjugateGradient::fused_spmv_dot, 4.5, spmv_bytes(), 3.0e6);
    auto ux = op("x", "CgFusedAxpy", &ConjugateGradient::fused_x, 3.3, 12.0 * n);
    auto ur = op("r", "CgFusedAxpyDot", &ConjugateGradient::fused_r, 3.5, 12.0 * n);
    auto up = op("p", "CgFusedXpay", &ConjugateGradient::fused_p, 3.3, 12.0 * n);
    g->start_then(sd);
    g->then(sd, ux); // alpha: the pq partials (and q for the r update)
    g->then(sd, ur);
    g->then(ur, up); // beta: the rr partials, and the new r
    g->then(ux, up); // p is overwritten after its readers (the SpMV through ux / ur)
    g->then_finish(up);
    return g;
  }
  auto sp = op("spmv", "CgSpmv", &ConjugateGradient::spmv, 4.0, spmv_bytes(), 3.0e6);
  auto dpq = op("dot_pq", "CgDot", &ConjugateGradient::dot_pq, 3.0, 8.0 * n);
  auto al = op("alpha", "CgScalar", &ConjugateGradient::alpha, 2.5, 0.0);
  auto ux = op("x", "CgAxpy", &ConjugateGradient::update_x, 3.0, 12.0 * n);
  auto ur = op("r", "CgAxpy", &ConjugateGradient::update_r, 3.0, 12.0 * n);
  auto drr = op("dot_rr", "CgDot", &ConjugateGradient::dot_rr, 3.0, 4.0 * n);
  auto be = op("beta", "CgScalar", &ConjugateGradient::beta, 2.5, 0.0);
  auto up = op("p", "CgXpay", &ConjugateGradient::update_p, 3.0, 12.0 * n);
  g->start_then(sp);
  g->then(sp, dpq);
  g->then(dpq, al);
  g->then(al, ux);
  g->then(al, ur);
  g->then(sp, ur); // q is written before the r update reads it
  g->then(ur, drr);
  g->then(drr, be); // beta also rewrites rr: after alpha read it (alpha -> r -> dot_rr -> beta)
  g->then(be, up);
  g->then(ux, up); // p is overwritten after both of its readers
  g->then(sp, up);
  g->then_finish(up);
  return g;
}

void ConjugateGradient::add_to_graph(Graph &g) {
  const std::string &p = a_.prefix;
  OpPtr top;
  if (a_.form == "choice" || a_.form == "all") {
    std::vector<OpPtr> alts = {std::make_shared<StaticCompoundOp>(p + "plain", form_graph(false)),
                               std::make_shared<StaticCompoundOp>(p + "fused", form_graph(true))};
    if (a_.form == "all") alts.push_back(std::make_shared<StaticCompoundOp>(p + "sr", sr_graph()));
    top = std::make_shared<StaticChoiceOp>(p + "form", alts);
  } else if (a_.form == "sr") {
    top = std::make_shared<StaticCompoundOp>(p + "sr", sr_graph());
  } else {
    top = std::make_shared<StaticCompoundOp>(p + a_.form, form_graph(a_.form == "fused"));
  }
  g.start_then(top);
  g.then_finish(top);
}

} // namespace tz
