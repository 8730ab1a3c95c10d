// orz_decode_drive.h -- what the host drivers of the device decoder share (host side only, templated on the backend).
//
// Six drivers launch DecodeMember / DecodeMemberCursor: decode_members_device (orz_decode_device.h), decode_members_to_device
// (orz_decode_index.h), decode_members_scatter (orz_decode_scatter.h), decode_members_planes (orz_planes.h), RangeReader::read and
// ::read_cached (orz_decode_range.h).
// Here is what is literally the same in all of them: the message of a failed member, the owner of a call's device buffers, the
// upload of a host container, the timing bracket, the loop over rounds of `slots` members and the launch of one round -- and
// decode_all, the whole sequence of the four one-shot drivers.  The three drivers with destinations in device memory (to_device,
// scatter, planes) also open the same way -- open_container: upload, index, host waits, the stats' sizes -- and the two with a
// destination per member or tensor close the same way -- read_statuses, one read and one wait; throw_first_bad -- and refuse the same
// destinations, each in its own words (check_destinations, DestinationNames).  What differs stays with its driver: where the bytes
// go, what is read back besides the statuses, and the readers' rules for zeroing a state that outlives the call.
//
// orz_decode_device.h includes this header below the decoder's types; include that one.
#pragma once
#include <algorithm>
#include <array>
#include <stdexcept>
#include <string>
#include <utility>
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

// The opening of a driver with destinations in device memory: the container where the kernels read it, `ix` (a DeviceIndex,
// orz_decode_index.h) built over it -- `want_arrays` as for its build() --, the host waits of both counted, `members` and the stats'
// sizes set.  Returns the container's device address.  What build() throws passes through, with only the upload's wait counted.
template <class BE, class IX, class Stats>
const uint8_t* open_container(DeviceBuffers<BE>& own, IX& ix, const uint8_t* src, size_t n, bool src_on_device, bool table, const uint64_t* offs,
                              const uint64_t* lens, size_t n_table, bool want_arrays, uint64_t& members, Stats& stats) {
    const uint8_t* d_src = upload_container(own, src, n, src_on_device, stats.host_waits);
    ix.build(d_src, n, table, offs, lens, n_table, want_arrays);
    stats.host_waits += ix.host_waits;
    members = ix.members;
    stats.members = ix.members; stats.in_bytes = n; stats.out_bytes = ix.total;
    return d_src;
}

// The closing: the M statuses behind the last launch, in one read and one host wait ...
template <class BE>
std::vector<uint32_t> read_statuses(BE& be, const uint32_t* d_status, uint64_t M, uint64_t& host_waits) {
    std::vector<uint32_t> status((size_t)M);
    be.d2h(status.data(), d_status, (size_t)M * 4);
    host_waits++;
    return status;
}
// ... and decode_status_error for the first member whose status is not kDecOk
inline void throw_first_bad(const uint32_t* status, uint64_t M) {
    for (uint64_t m = 0; m < M; m++)
        if (status[m] != kDecOk) throw decode_status_error(m, status[m]);
}

// How a driver speaks of its destinations: "no destination for member 3" or "no destination 3 for its planes", "the destination of
// member 3" or "destination 3", "the destinations of members 2 and 5" or "destinations 2 and 5".
struct DestinationNames {
    const char *missing, *missing_end, *one, *two;
};
// The destinations that have bytes -- `iv`: (address, index) in index order, sorted here; caps[index]: their capacities -- may be
// written: none null, none wrapping the address space, none overlapping the next (whole capacities count), none overlapping a
// device-resident container.  Throws std::runtime_error for the first that may not, a null one before any other.
inline void check_destinations(std::vector<std::pair<uint64_t, uint64_t>>& iv, const uint64_t* caps, const uint8_t* src, size_t n, bool src_on_device,
                               const DestinationNames& names) {
    const auto refuse = [](const std::string& what) { return std::runtime_error("invalid argument: " + what); };
    for (const auto& d : iv)
        if (!d.first) throw refuse(names.missing + std::to_string(d.second) + names.missing_end);
    std::sort(iv.begin(), iv.end());
    for (size_t i = 0; i < iv.size(); i++) {
        const uint64_t a = iv[i].first, k = iv[i].second, cap = caps[k];
        if (cap > ~a) throw refuse(names.one + std::to_string(k) + " wraps the address space");
        if (i + 1 < iv.size() && iv[i + 1].first < a + cap)
            throw refuse(names.two + std::to_string(std::min(k, iv[i + 1].second)) + " and " + std::to_string(std::max(k, iv[i + 1].second)) + " overlap");
        const uint64_t s = (uint64_t)(uintptr_t)src;
        if (src_on_device && n && cap && a < s + n && s < a + cap) throw refuse(std::string("the container and ") + names.one + std::to_string(k) + " overlap");
    }
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
