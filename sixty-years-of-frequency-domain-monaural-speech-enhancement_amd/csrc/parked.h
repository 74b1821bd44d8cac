// What every parked object is (se_stream_state in stream_state.hip, ResamplerState in k_resample.hip): a host manifest of the owner's
// kind + one payload that lives on one device at a time, or on the host as an imported image, or both.  The rules, once:
//   - a call on another hipStream than the last one waits for the event the last one left (wait), and every call leaves it (mark);
//   - what lives on a device is released with that device current, behind the last use (drop_side);
//   - an imported image is uploaded once per device it is restored on, behind the last use (upload_host);
//   - export reads the host image, or the device behind the last use; import replaces the image and touches no device.
// How a payload is sized is the owner's business (fresh_payload takes bytes).  Host code over the HIP runtime; no kernels.
#pragma once
#include "hip_owned.h"
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace se {

struct DeviceScope {      // a call on an object alone: its device is current while the call runs (dev < 0: no device yet, nothing to do)
    int prev = -1;
    explicit DeviceScope(int dev) {
        if (dev < 0) return;
        int cur = -1;
        SE_HIP(hipGetDevice(&cur));
        if (cur != dev) {
            SE_HIP(hipSetDevice(dev));
            prev = cur;
        }
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

struct Parked {
    bool filled = false;
    int device = -1;                      // the device the side lives on
    bool dev_valid = false;               // the side holds the payload of the manifest (false after an import, until the first upload)
    std::vector<uint8_t> host;            // payload of an imported image (kept: another device may restore it too)
    struct Side {                         // what belongs to one device; made with the first payload (an owner may keep more here: make_side)
        DevBuf<uint8_t> dev;
        size_t bytes = 0;
        Event ev_use;
        virtual ~Side() = default;
    };
    std::unique_ptr<Side> side;
    // the hipStream the object was last used on: a call on another one is ordered behind it
    bool has_use = false;
    hipStream_t use_st = nullptr;

    virtual ~Parked() = default;
    virtual std::unique_ptr<Side> make_side() const { return std::unique_ptr<Side>(new Side()); }

    bool has_payload() const { return side && side->dev; }
    bool resident() const { return dev_valid && has_payload(); }      // the snapshot's payload is on `device`
    bool on_device(int dev) const { return resident() && device == dev; }

    void wait(hipStream_t st) {
        if (has_use && use_st != st) SE_HIP(hipStreamWaitEvent(st, side->ev_use.get(), 0));
    }
    void mark(hipStream_t st) {
        SE_HIP(hipEventRecord(side->ev_use.get(), st));
        has_use = true;
        use_st = st;
    }
    // the host waits for the last use (with the side's device current)
    void sync_use() {
        if (!has_use) return;
        DeviceScope ds(device);
        SE_HIP(hipEventSynchronize(side->ev_use.get()));
        has_use = false;
    }
    void drop_side() {
        if (side) {
            DeviceScope ds(device);
            if (has_use) (void)hipEventSynchronize(side->ev_use.get());
            side.reset();
        }
        has_use = false;
        dev_valid = false;
    }
    // a new payload buffer of `bytes` on `dev` (current), its contents undefined; a side on another device goes first
    void fresh_payload(size_t bytes, int dev) {
        if (side && device != dev) drop_side();
        if (!side) side = make_side();
        DevBuf<uint8_t> fresh;
        fresh.alloc(bytes);
        side->dev = std::move(fresh);
        side->bytes = bytes;
        device = dev;
        dev_valid = false;
    }
    // the imported image -> the payload its owner has just sized on the current device: once, until the object is saved into again.
    // Behind the last use, which is nothing for an image that was imported and never used
    void upload_host() {
        SE_CHECK(has_payload() && host.size() <= side->bytes, "parked object: host image larger than its payload");
        sync_use();
        SE_HIP(hipMemcpy(side->dev.get(), host.data(), host.size(), hipMemcpyHostToDevice));
        dev_valid = true;
    }
    // the first `bytes` of the payload, from the imported image or else from the device behind the last use.  That there is a payload
    // of the manifest's size is the caller's refusal to make, in its own words; the guard keeps the copy inside what the object holds
    void export_payload(uint8_t* out, size_t bytes) {
        SE_CHECK(host.empty() ? has_payload() && dev_valid && bytes <= side->bytes : bytes <= host.size(), "parked object: no payload of that size");
        if (!host.empty()) {
            std::memcpy(out, host.data(), bytes);
            return;
        }
        sync_use();
        DeviceScope ds(device);
        if (bytes > 0) SE_HIP(hipMemcpy(out, side->dev.get(), bytes, hipMemcpyDeviceToHost));
    }
    // the tail of an import (the owner has replaced its manifest): nothing on a device is valid any more
    void adopt_image(std::vector<uint8_t>&& image) {
        host = std::move(image);
        filled = true;
        dev_valid = false;
    }
    // the tail of a save or a gather: the object holds the owner's new manifest, its payload on the device (or none: on_dev false)
    void set_saved(bool on_dev = true) {
        filled = true;
        dev_valid = on_dev;
        host.clear();
        host.shrink_to_fit();
    }
};

// The parts of a concat or a join (T: a Parked with a manifest `man`): none null, none dst, none empty, under 2^24 rows in all;
// each(p, part) makes the caller's own checks of part p where the loop stands.  what: "stream state" / "resampler state"
template <typename T, typename F>
std::vector<T*> collect_parts(const T* dst, const T* const* cparts, int32_t n_parts, const std::string& fn, const char* what, F&& each) {
    SE_CHECK(n_parts >= 1, fn + "n_parts " + std::to_string(n_parts) + ": at least one part has to be given");
    std::vector<T*> parts;
    int64_t total = 0;
    for (int32_t p = 0; p < n_parts; ++p) {
        T* s = const_cast<T*>(cparts[p]);      // (the uploaded payload is a cache of the object)
        const std::string name = "parts[" + std::to_string(p) + "]";
        SE_CHECK(s, fn + name + " is null");
        SE_CHECK(s != dst, fn + "dst == " + name + ": the rows are read while they are written");
        SE_CHECK(s->filled, fn + name + ": the " + what + " object is empty");
        each(p, s);
        total += s->man.batch;
        SE_CHECK(total < (1 << 24), fn + "too many rows");
        parts.push_back(s);
    }
    return parts;
}
// ... and their rows in order, as (part, row)
template <typename T>
std::vector<int2> part_rows(const std::vector<T*>& parts) {
    std::vector<int2> map;
    for (size_t p = 0; p < parts.size(); ++p)
        for (int32_t r = 0; r < parts[p]->man.batch; ++r) map.push_back(make_int2((int)p, r));
    return map;
}

}  // namespace se
