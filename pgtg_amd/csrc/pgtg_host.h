// pgtg_amd/csrc/pgtg_host.h -- all that a translation unit other than pgtg_env.hip may know about a handle.
//
// struct pgtg_handle is defined in pgtg_env.hip alone and stays an incomplete type everywhere else.  The three
// functions below are defined there, next to it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/pgtg.h"

// (linked between the library's objects, not exported from it: the library's surface is include/pgtg.h)
#define PGTG_INTERNAL __attribute__((visibility("hidden")))

// What an entry point outside pgtg_env.hip launches with: the handle's device and stream, its per-env error
// bytes (nullptr before they are allocated) and its env count.
struct pgtg_host {
  int device;
  hipStream_t stream;
  uint8_t* err_bytes;
  uint64_t n;
};
PGTG_INTERNAL pgtg_host pgtg_host_of(const pgtg_handle* h);

// sets the handle's error string to `m`; returns `code`
PGTG_INTERNAL int fail(pgtg_handle* h, int code, const std::string& m);

// sets the handle's error string to "<expr>: <what e means>"; returns PGTG_E_DEVICE
PGTG_INTERNAL int pgtg_hip_failed(pgtg_handle* h, hipError_t e, const char* expr);

// `x` is a HIP call: where it fails, the enclosing function returns PGTG_E_DEVICE with the error string set
#define HIPCHK(h, x)                                               \
  do {                                                             \
    hipError_t e_ = (x);                                           \
    if (e_ != hipSuccess) return pgtg_hip_failed((h), e_, #x);     \
  } while (0)
