// top_order.hpp — the order of ORDER BY <aggregate> LIMIT k over groups (contract: include/aqe_hip.h, aqe_top_spec), shared by
// the device selection of wide_group.hip and the host selection of top_host.cpp.  Plain C++: no HIP header is needed here.
//
// A ranked group gets a 64-bit RANK KEY such that a smaller key is a better rank in the direction asked for: the
// order-preserving key of its value (okey of device_common.hpp; -0.0 folded into +0.0), complemented for a descending order.
// Every non-NaN value's key lies in [0x000f..., 0xfff0...] (-inf .. +inf), so its complement does too: the two largest 64-bit
// numbers are free for a NaN value (last among the ranked in both directions) and for a group that is not ranked at all.
// Ties are broken by the bin (the position in an ascending list): the COMPOSITE (rank key, bin) is unique per group.
#pragma once
#include <cstdint>

namespace aqe {

constexpr uint64_t kTopUnranked = ~0ull;       // visited == 0 or n == 0: above every ranked key
constexpr uint64_t kTopNaN = ~0ull - 1ull;     // a NaN value: the largest rankable key
constexpr uint64_t kTopLargestNumber = 0xfff0000000000000ull;  // okey(+inf) and ~okey(-inf)

// okey of device_common.hpp over the bits of a double: a < b as doubles <=> okey_of_bits(a) < okey_of_bits(b) as integers, NaN
// aside; -0.0 and +0.0 are one value.  The one copy both selections use: the device passes __double_as_longlong(value), the
// host the bytes of the double.
constexpr uint64_t okey_of_bits(uint64_t b) {
    if ((b << 1) == 0) b = 0;  // either zero
    return (b >> 63) ? ~b : (b | (1ull << 63));
}

static_assert(okey_of_bits(0x8000000000000000ull) == okey_of_bits(0), "-0.0 and +0.0 are one value");
static_assert(okey_of_bits(0x7ff0000000000000ull) == kTopLargestNumber && ~okey_of_bits(0xfff0000000000000ull) == kTopLargestNumber,
              "every number's key, and its complement, lies below the two keys kept free");
static_assert(okey_of_bits(0xbff0000000000000ull) < okey_of_bits(0) && okey_of_bits(0) < okey_of_bits(0x3ff0000000000000ull), "-1 < 0 < 1");

// ok: okey_of_bits of a value that is not NaN.
constexpr uint64_t top_rank_key(uint64_t ok, bool descending) { return descending ? ~ok : ok; }

// (key a, bin a) before (key b, bin b)
constexpr bool top_before(uint64_t ka, uint32_t ba, uint64_t kb, uint32_t bb) { return ka < kb || (ka == kb && ba < bb); }

}  // namespace aqe
