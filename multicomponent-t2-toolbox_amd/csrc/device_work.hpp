// device_work.hpp -- the one owner of a C-ABI call's device work space (the imaging entries; plan-lifetime memory is plan.hpp's business).
// take() states the layout once: the pieces, each rounded up to 256 bytes, in the order they are named.  alloc() makes the one block, after
// which a piece reads as its pointer.  ok() latches the first HIP error.  finish() waits for the stream, gives the block back and reports; the
// destructor does the same on every other return, so a block that a kernel still uses cannot be freed.  A block the caller supplied is neither
// waited for nor freed.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/met2_hip.h"
#include "abi_common.hpp"

namespace {

class DeviceWork {
    hipStream_t st_;
    char *block_ = nullptr;
    size_t bytes_ = 0;
    bool callers_ = false;                // the block is the caller's
    hipError_t err_ = hipSuccess;

    void release()                        // not before the stream is through with the block
    {
        if (callers_) return;
        ok(hipStreamSynchronize(st_));
        (void)hipFree(block_);
        block_ = nullptr;
    }

public:
    template <class T> struct Piece {     // reads as the piece's T * once alloc() has run
        const DeviceWork *w;
        size_t off, bytes;                // bytes: the rounded size
        operator T *() const { return (T *)(w->block_ + off); }
        T *operator->() const { return *this; }
    };

    explicit DeviceWork(hipStream_t st) : st_(st) {}
    DeviceWork(const DeviceWork &) = delete;
    ~DeviceWork() { if (block_) release(); }

    template <class T> Piece<T> take(size_t count)     // the next piece: count elements of T
    {
        const Piece<T> p{this, bytes_, (count * sizeof(T) + 255) / 256 * 256};
        bytes_ += p.bytes;
        return p;
    }

    // one block for all pieces: the caller's, if there is one (it holds what was taken, at least), else a new one
    bool alloc(void *callers = nullptr)
    {
        callers_ = callers != nullptr;
        block_ = (char *)callers;
        return callers_ || !bytes_ || ok(hipMalloc((void **)&block_, bytes_));
    }

    bool ok(hipError_t e = hipSuccess) { if (err_ == hipSuccess) err_ = e; return err_ == hipSuccess; }

    // what every entry does last: the launches' error, wait, give the block back, report.  Host copies are read after MET2_OK only.
    int finish(const char *who)
    {
        if (ok()) ok(hipGetLastError());
        release();
        return ok() ? MET2_OK : fail(MET2_E_HIP, std::string(who) + ": " + hipGetErrorString(err_));
    }
};

}  // namespace
