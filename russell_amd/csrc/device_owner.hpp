// device_owner.hpp -- move-only owners of HIP resources: device memory, pinned host memory, streams, events, the captured graph.
// An owner frees what it holds when it is destroyed, reset or assigned; a struct of owners is released by assigning a fresh one.
// It converts implicitly to the raw handle, so kernel arguments and pointer arithmetic read as with a plain pointer.
#pragma once
#include <hipmf_device_rt.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <vector>

namespace hipmf {

struct FreeDevice {
    void operator()(void *p) const { (void)hipFree(p); }
};
struct FreePinned {
    void operator()(void *p) const { (void)hipHostFree(p); }
};
struct DestroyStream {
    void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
};
struct DestroyEvent {
    void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
};

template <class H, class Release>
class Owner {
  public:
    Owner() = default;
    Owner(const Owner &) = delete;
    Owner &operator=(const Owner &) = delete;
    Owner(Owner &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owner &operator=(Owner &&o) noexcept {
        if (this != &o) reset(o.h_), o.h_ = nullptr;
        return *this;
    }
    ~Owner() { reset(); }
    // frees what it holds and takes h
    void reset(H h = nullptr) {
        if (h_) Release()(h_);
        h_ = h;
    }
    // frees what it holds; the address of the empty handle, for the create calls of HIP
    H *put() {
        reset();
        return &h_;
    }
    H get() const { return h_; }
    operator H() const { return h_; }

  private:
    H h_ = nullptr;
};

template <class T, class Release>
class Array : public Owner<T *, Release> {
  public:
    // count elements (not zeroed); frees what it held first
    hipError_t alloc(size_t count) {
        void **p = (void **)this->put();
        if constexpr (std::is_same<Release, FreePinned>::value) return hipHostMalloc(p, sizeof(T) * count);
        else return hipMalloc(p, sizeof(T) * count);
    }
    // a device copy of v (at least one element is allocated)
    template <class A>
    hipError_t upload(const std::vector<T, A> &v) {
        hipError_t e = alloc(std::max<size_t>(v.size(), 1));
        if (e == hipSuccess && !v.empty()) e = hipMemcpy(this->get(), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        return e;
    }
};

template <class T>
using DeviceArray = Array<T, FreeDevice>;
template <class T>
using PinnedArray = Array<T, FreePinned>;
using StreamOwner = Owner<hipStream_t, DestroyStream>;
using EventOwner = Owner<hipEvent_t, DestroyEvent>;
#ifndef HIPMF_EMULATED
struct DestroyGraphExec {
    void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); }
};
using GraphExecOwner = Owner<hipGraphExec_t, DestroyGraphExec>;
#endif

} // namespace hipmf
