// orz_decode_drive.h -- what the host drivers of the device decoder share (host side only, templated on the backend).
//
// Six drivers launch DecodeMember / DecodeMemberCursor: decode_members_device (orz_decode_device.h), decode_members_to_device
// (orz_decode_index.h), decode_members_scatter (orz_decode_scatter.h), decode_members_planes (orz_planes.h), RangeReader::read and
// ::read_cached (orz_decode_range.h).
// Here is what is literally the same in all of them: the message of a failed member, the owner of a call's device buffers, the
// upload of a host container, the timing bracket, the loop over rounds of `slots` members and the launch of one round -- and
// decode_all, the whole sequence of the four one-shot drivers.  What differs stays with its driver: where the bytes go, how the
// statuses come back, and the readers' rules for zeroing a state that outlives the call.
//
// orz_decode_device.h includes this header below the decoder's types; include that one.
#pragma once
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

namespace orz {

// what a driver throws for the first member whose status is not kDecOk
inline std::runtime_error decode_status_error(uint64_t member, uint32_t status) {
    return std::runtime_error(status == kDecDeepTable ? "member with a 16-bit Huffman table: use the host decoder"
                                                      : "invalid orz data (member " + std::to_string(member) + ", status " + std::to_string(status) + ")");
}

// The device buffers of one call, freed in the order they were made on every way out.
template <class BE>
struct DeviceBuffers {
    BE& be;
    std::vector<void*> held;
    explicit DeviceBuffers(BE& b) : be(b) {}
    DeviceBuffers(const DeviceBuffers&) = delete;
    DeviceBuffers& operator=(const DeviceBuffers&) = delete;
    ~DeviceBuffers() { for (void* p : held) if (p) be.free(p); }
    template <class T>
    T* alloc(size_t n, bool zero = true) {
        held.reserve(held.size() + 1);  // (nothing throws between the allocation and its entry)
        T* p = be.template alloc<T>(n, zero);
        held.push_back(p);
        return p;
    }
};

// The container where the kernels can read it: a host container is uploaded into a buffer of `own` (one host wait).
template <class BE>
const uint8_t* upload_container(DeviceBuffers<BE>& own, const uint8_t* src, size_t n, bool src_on_device, uint64_t& host_waits) {
    if (src_on_device) return src;
    uint8_t* up = own.template alloc<uint8_t>(n, false);
    own.be.h2d(up, src, n);
    host_waits++;
    return up;
}

// Event timing on from here to the end of the scope, also when the scope is left by an exception.  finish() waits for the
// streams and returns the milliseconds per slot (2 = the decode launches, 1 = the readers' gather).
template <class BE>
struct TimedBracket {
    struct Off {  // (a member, so that timing goes off too when the constructor's collect_timed throws)
        BE& be;
        ~Off() { be.set_timing(false); }
    } off;
    uint64_t nl = 0;
    explicit TimedBracket(BE& be) : off{be} {
        be.set_timing(true);
        be.collect_timed(&nl);  // (drops what an earlier call left)
    }
    std::array<double, 4> finish() {
        std::array<double, 4> ms;
        uint64_t nby[4];
        off.be.collect_timed(&nl, ms.data(), nby);
        return ms;
    }
};

// members in flight at once: at least one, no more than there are to decode
inline uint32_t clamp_slots(uint64_t need, uint32_t slots) { return slots == 0 ? 1 : slots > need ? (uint32_t)need : slots; }

// round(first, count) for members first .. first + count - 1 of `need`, `slots` at a time
template <class F>
void decode_rounds(uint64_t need, uint32_t slots, F&& round) {
    slots = clamp_slots(need, slots);
    for (uint64_t first = 0; first < need; first += slots) round((uint32_t)first, need - first < slots ? (uint32_t)(need - first) : slots);
}

// one round: K (DecodeMember or DecodeMemberCursor) over a.count members, timed in slot 2
template <class K, class BE>
void launch_decode(BE& be, const DecodeArgs& a, uint64_t& launches) {
    be.timed_begin(2);  // (a slot that is recorded without profile mode)
    be.launch_waves(a.count, K{a}, K::lds_bytes());
    be.timed_end(2);
    launches++;
}

// All M > 0 members of `a` (first / count are filled in here), whole, `slots` at a time: the one-shot drivers' sequence.  The
// state is a.state when the caller made it (zeroed, clamp_slots(M, slots) blobs), else a zeroed buffer of `own`; every later
// round zeroes it again.  Sets stats.launches and stats.kernel_ms; the statuses are the caller's to read.
template <class BE>
void decode_all(BE& be, DecodeArgs a, uint64_t M, uint32_t slots, DeviceBuffers<BE>& own, DecodeStats& stats) {
    slots = clamp_slots(M, slots);
    const size_t state_bytes = (size_t)slots * DecodeLayout::kBytes;
    if (!a.state) a.state = own.template alloc<uint8_t>(state_bytes);
    TimedBracket<BE> timed(be);
    decode_rounds(M, slots, [&](uint32_t first, uint32_t count) {
        if (first) be.memset(a.state, 0, state_bytes);  // (alloc zeroes the first round)
        a.first = first;
        a.count = count;
        launch_decode<DecodeMember>(be, a, stats.launches);
    });
    stats.kernel_ms = timed.finish()[2];
}

}  // namespace orz
