// Diagnostics build of the fp32 skinny GEMM family (libultrafnd_hip_diag.so; never loaded by the product package): the three
// launchers with a problem array given by the caller, each reporting the instantiation it launched and its grid, and the
// host-only validation + choice on its own.  Used by tests/test_gemm_f32_cases.py and tests/test_gpu_gemm_f32.py.
#define UFND_DIAG 1
#include "../gemm_f32.hip"

namespace {
template <class Prob>
int diag_run(const Prob* probs, int nprob, const ufnd_step_state* state, int* form, int* grid, void* stream_) {
  GemmF32Form f = GEMM_F32_FORMS;
  const int rc = run(probs, nprob, state, (hipStream_t)stream_, &f, grid);
  if (form) *form = (int)f;
  return rc;
}
// validation and choice only
template <class Prob>
int diag_plan(const void* probs, int nprob, GemmF32Form* form, int* grid) {
  GemmArgs<Prob> a;
  return choose((const Prob*)probs, nprob, a, form, grid);
}
}  // namespace

extern "C" int ufnd_diag_gemm_f32_nt(const NtProb* probs, int nprob, const ufnd_step_state* state, int* form, int* grid, void* stream_) {
  return diag_run(probs, nprob, state, form, grid, stream_);
}
extern "C" int ufnd_diag_gemm_f32_nn(const NnProb* probs, int nprob, const ufnd_step_state* state, int* form, int* grid, void* stream_) {
  return diag_run(probs, nprob, state, form, grid, stream_);
}
extern "C" int ufnd_diag_gemm_f32_tn(const TnProb* probs, int nprob, int* form, int* grid, void* stream_) {
  return diag_run(probs, nprob, nullptr, form, grid, stream_);
}

// Validation and choice only: kind 0 = nt (NtProb), 1 = nn (NnProb), 2 = tn (TnProb).  Nothing is launched and no operand is
// dereferenced -- the pointers only have to carry the alignment of the real ones -- so this answers on a machine without a GPU.
extern "C" int ufnd_diag_gemm_f32_plan(int kind, const void* probs, int nprob, int* form, int* grid) {
  UFND_REQUIRE(form && grid, "gemm_f32_plan: null result pointer");
  UFND_REQUIRE(kind >= 0 && kind <= 2, "gemm_f32_plan: kind %d", kind);
  GemmF32Form f = GEMM_F32_FORMS;
  const int rc = kind == 0 ? diag_plan<NtProb>(probs, nprob, &f, grid) : kind == 1 ? diag_plan<NnProb>(probs, nprob, &f, grid) : diag_plan<TnProb>(probs, nprob, &f, grid);
  *form = (int)f;
  return rc;
}

// sizeof of the three problem structures and of the form enum's range (the ctypes mirrors are checked against them)
extern "C" void ufnd_diag_gemm_f32_sizes(int* out4) {
  out4[0] = (int)sizeof(NtProb);
  out4[1] = (int)sizeof(NnProb);
  out4[2] = (int)sizeof(TnProb);
  out4[3] = (int)GEMM_F32_FORMS;
}
