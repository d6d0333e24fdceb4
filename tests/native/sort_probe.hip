// Test infrastructure (tests/sort_probe.py, tests/test_gpu_sort.py), not part of the C-ABI: a thin
// extern "C" door to the radix sort of fm_sort.hip, so the suite can compare it with a stable host
// sort directly.  It runs the kernels that ship: this file holds no kernel and no copy of the sort,
// fmhip::radix_sort_* and DevBuf come from the built libfm_hip.so it is linked against.
//
// A handle owns one SortWork and one non-blocking stream, as a context does, so a sequence of sorts
// reuses the same work buffers.  Every call copies its inputs into fresh device buffers, sorts,
// synchronises and copies the results back; the input buffers are read back too (a batch's col / ent
// are sorted again at every step, so the sort must leave them alone), and the final buffers, when
// used, sit between guard words.  No exception crosses the boundary.
#include <cstring>
#include <exception>
#include <string>
#include <vector>

#include "../../fm_spark_amd/csrc/fm_internal.h"

namespace {

constexpr int kGuard = 64;  // guard words (uint32) before and after the final keys and the final payloads
constexpr uint32_t kGuardPattern = 0xA5C3F00Du;

struct Probe {
  fmhip::SortWork work;
  hipStream_t st = nullptr;
};

thread_local std::string g_msg;

template <class F>
int guarded(F&& f) {
  try {
    g_msg.clear();
    return f();
  } catch (const fmhip::Error& e) {
    g_msg = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    g_msg = e.what();
    return FM_ERR_HIP;
  } catch (...) {
    g_msg = "unknown exception";
    return FM_ERR_HIP;
  }
}

void fill_guards(std::vector<uint32_t>& h, size_t body_words) {
  for (int i = 0; i < kGuard; ++i) {
    h[i] = kGuardPattern ^ (uint32_t)i;
    h[kGuard + body_words + i] = kGuardPattern ^ (uint32_t)(kGuard + i);
  }
}

bool guards_intact(const std::vector<uint32_t>& h, size_t body_words) {
  for (int i = 0; i < kGuard; ++i) {
    if (h[i] != (kGuardPattern ^ (uint32_t)i)) return false;
    if (h[kGuard + body_words + i] != (kGuardPattern ^ (uint32_t)(kGuard + i))) return false;
  }
  return true;
}

}  // namespace

extern "C" {

// kinds of sort_probe_sort
enum { kPairs32 = 0, kPairs64 = 1, kPairs64Bits = 2 };

const char* sort_probe_last_error(void) { return g_msg.c_str(); }

int sort_probe_create(void** out) {
  return guarded([&]() -> int {
    FM_REQUIRE(out, "null argument");
    *out = nullptr;
    Probe* p = new Probe();
    hipError_t e = hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete p;
      throw fmhip::Error{FM_ERR_HIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e)};
    }
    *out = p;
    return FM_OK;
  });
}

void sort_probe_destroy(void* h) {
  Probe* p = static_cast<Probe*>(h);
  if (!p) return;
  (void)guarded([&]() -> int {
    if (p->st) {
      (void)hipStreamSynchronize(p->st);
      (void)hipStreamDestroy(p->st);
    }
    delete p;  // the SortWork's buffers go with it
    return FM_OK;
  });
}

// kind kPairs32: keys (uint32) with vals (uint32 [n], or NULL for the implicit index) by bits [0, hi_bit);
//      kPairs64: vals uint2 [n], by bits [0, hi_bit); use_final: the last pass writes the guarded final buffers;
//      kPairs64Bits: vals uint2 [n], by bits [lo_bit, hi_bit), always into the guarded final buffers.
// The device keys start key_misalign_words (0..3) words past a 16-byte boundary.  out_keys [n] and
// out_vals [n] (uint32 or uint2) receive the result; *inputs_unchanged = the device inputs still
// equal what was uploaded; *guard_ok = the guard words around the final buffers survived (1 when no
// final buffer is used).
int sort_probe_sort(void* h, int kind, const uint32_t* keys, const void* vals, int64_t n, int lo_bit, int hi_bit,
                    int key_misalign_words, int use_final, uint32_t* out_keys, void* out_vals,
                    int* inputs_unchanged, int* guard_ok) {
  return guarded([&]() -> int {
    using namespace fmhip;
    Probe* p = static_cast<Probe*>(h);
    FM_REQUIRE(p && inputs_unchanged && guard_ok, "null argument");
    FM_REQUIRE(kind == kPairs32 || kind == kPairs64 || kind == kPairs64Bits, "unknown sort kind");
    FM_REQUIRE(key_misalign_words >= 0 && key_misalign_words <= 3, "key misalignment out of range");
    FM_REQUIRE(kind != kPairs32 || !use_final, "the 4-byte payload sort has no final buffers");
    FM_REQUIRE(kind == kPairs32 || vals || n <= 0, "the 8-byte payload sort needs payloads");
    *inputs_unchanged = 0;
    *guard_ok = 0;
    const size_t m = n > 0 ? (size_t)n : 0;  // what is copied; n itself goes to the library as given
    FM_REQUIRE(m == 0 || (keys && out_keys && out_vals), "null argument");
    const size_t vw = kind == kPairs32 ? 1 : 2;  // payload words
    const bool fin = kind == kPairs64Bits || use_final;
    hipStream_t st = p->st;

    DevBuf dkeys, dvals, fkeys, fvals;
    dkeys.ensure(sizeof(uint32_t) * (m + 8));  // hipMalloc aligns far beyond 16 bytes
    FM_REQUIRE((reinterpret_cast<uintptr_t>(dkeys.p) & 15u) == 0, "device allocation not 16-byte aligned");
    uint32_t* kin = dkeys.as<uint32_t>() + key_misalign_words;
    if (m) FM_HIP_CHECK(hipMemcpyAsync(kin, keys, sizeof(uint32_t) * m, hipMemcpyHostToDevice, st));
    uint32_t* vin = nullptr;
    if (vals) {
      dvals.ensure(sizeof(uint32_t) * vw * (m + 8));
      vin = dvals.as<uint32_t>();
      if (m) FM_HIP_CHECK(hipMemcpyAsync(vin, vals, sizeof(uint32_t) * vw * m, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> gk, gv;
    uint32_t* fk = nullptr;
    uint32_t* fv = nullptr;
    if (fin) {
      gk.assign(2 * kGuard + m, 0xDEADBEEFu);
      gv.assign(2 * kGuard + 2 * m, 0xDEADBEEFu);
      fill_guards(gk, m);
      fill_guards(gv, 2 * m);
      fkeys.ensure(sizeof(uint32_t) * gk.size());
      fvals.ensure(sizeof(uint32_t) * gv.size());
      FM_HIP_CHECK(hipMemcpyAsync(fkeys.p, gk.data(), sizeof(uint32_t) * gk.size(), hipMemcpyHostToDevice, st));
      FM_HIP_CHECK(hipMemcpyAsync(fvals.p, gv.data(), sizeof(uint32_t) * gv.size(), hipMemcpyHostToDevice, st));
      fk = fkeys.as<uint32_t>() + kGuard;
      fv = fvals.as<uint32_t>() + kGuard;
    }
    FM_HIP_CHECK(hipStreamSynchronize(st));

    const uint32_t* ok = nullptr;
    const void* ov = nullptr;
    if (kind == kPairs32) {
      const uint32_t* o32 = nullptr;
      radix_sort_pairs(p->work, kin, vin, n, hi_bit, st, &ok, &o32);
      ov = o32;
    } else if (kind == kPairs64) {
      const uint2* o64 = nullptr;
      radix_sort_pairs64(p->work, kin, reinterpret_cast<const uint2*>(vin), n, hi_bit, st, &ok, &o64, fk,
                         reinterpret_cast<uint2*>(fv));
      ov = o64;
    } else {
      radix_sort_pairs64_bits(p->work, kin, reinterpret_cast<const uint2*>(vin), n, lo_bit, hi_bit, st, fk,
                              reinterpret_cast<uint2*>(fv));
      ok = fk;
      ov = fv;
    }
    FM_HIP_CHECK(hipStreamSynchronize(st));

    if (fin) {  // the results are read from the final buffers themselves, guards and all
      FM_HIP_CHECK(hipMemcpyAsync(gk.data(), fkeys.p, sizeof(uint32_t) * gk.size(), hipMemcpyDeviceToHost, st));
      FM_HIP_CHECK(hipMemcpyAsync(gv.data(), fvals.p, sizeof(uint32_t) * gv.size(), hipMemcpyDeviceToHost, st));
      FM_HIP_CHECK(hipStreamSynchronize(st));
      *guard_ok = guards_intact(gk, m) && guards_intact(gv, 2 * m) ? 1 : 0;
      if (m) {
        // (with final buffers the library's returned pointers must be the final buffers)
        FM_REQUIRE(kind == kPairs64Bits || (ok == fk && ov == (const void*)fv),
                   "the sort did not return its final buffers");
        std::memcpy(out_keys, gk.data() + kGuard, sizeof(uint32_t) * m);
        std::memcpy(out_vals, gv.data() + kGuard, sizeof(uint32_t) * 2 * m);
      }
    } else {
      *guard_ok = 1;
      if (m) {
        FM_REQUIRE(ok && ov, "the sort returned no output");
        FM_HIP_CHECK(hipMemcpyAsync(out_keys, ok, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, st));
        FM_HIP_CHECK(hipMemcpyAsync(out_vals, ov, sizeof(uint32_t) * vw * m, hipMemcpyDeviceToHost, st));
        FM_HIP_CHECK(hipStreamSynchronize(st));
      }
    }

    bool same = true;
    if (m) {
      std::vector<uint32_t> back(vw * m > m ? vw * m : m);
      FM_HIP_CHECK(hipMemcpyAsync(back.data(), kin, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, st));
      FM_HIP_CHECK(hipStreamSynchronize(st));
      same = std::memcmp(back.data(), keys, sizeof(uint32_t) * m) == 0;
      if (vin) {
        FM_HIP_CHECK(hipMemcpyAsync(back.data(), vin, sizeof(uint32_t) * vw * m, hipMemcpyDeviceToHost, st));
        FM_HIP_CHECK(hipStreamSynchronize(st));
        same = same && std::memcmp(back.data(), vals, sizeof(uint32_t) * vw * m) == 0;
      }
    }
    *inputs_unchanged = same ? 1 : 0;
    return FM_OK;
  });
}

}  // extern "C"
