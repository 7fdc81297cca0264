// zone_probe.hpp — the device side of the zone map over a time-offset array, shared by the sweeps that leave cold tiles unread
// (k_window of time_window.hip, k_window_groups of window_group.hip): the zone, a tile's place in its family as visit_tile
// decodes it, and the verdict on a tile in flight.  The map itself — k_time_zones, its cache by array pointer — stays with
// time_window.hip (ensure_zones of host.hpp).
#pragma once

#include "device_common.hpp"

namespace aqe {

constexpr unsigned kZoneShift = 10, kZoneRows = 1u << kZoneShift;  // elements of the time array per zone
static_assert(kZoneRows == 64 * 16, "one wave per zone, 16 elements per lane");

struct Zone {
    int32_t min, max;
};

namespace {

// A tile's place in its family, as visit_tile decodes it.
struct TileGeom {
    u64 j, seg_len, step, seg_ord0, ord_lo, ord_hi, row_base, col0, pitch;
    int form;  // 0 dense (two ordinals per lane and load), 1 linear (pages), 2 strided
};
template <typename FamPtr>
__device__ __forceinline__ TileGeom tile_geom(const SweepCommon& sw, FamPtr fams, u64 t) {
    const auto& F = fams[find_family(fams, sw.nfam, t)];
    const u64 lt = t - F.tile_begin;
    u64 seg, j;
    if (F.tiles_per_seg == 0) { seg = F.seg_lo; j = F.j_lo + lt; }
    else { seg = F.seg_lo + lt / F.tiles_per_seg; j = lt % F.tiles_per_seg; }
    TileGeom g;
    g.j = j;
    g.seg_len = F.seg_len;
    g.step = F.step;
    g.seg_ord0 = seg * F.seg_len;
    g.ord_lo = F.ord_lo;
    g.ord_hi = F.ord_hi;
    g.row_base = F.row0 + seg * F.pitch - sw.shard_lo;
    g.col0 = F.row0 - sw.shard_lo;
    g.pitch = F.pitch;
    g.form = (sw.dense16 && is_dense16(F.step, F.flags, F.seg_len)) ? 0 : (F.flags & kFamLinear) ? 1 : 2;
    return g;
}

// The verdict on a tile, in flight: the lane's zone of the tile's element range (when the range is one the map can judge).
struct Probe {
    bool can;     // wave-uniform: the range is valid and spans at most 64 zones
    bool active;  // this lane holds a zone of it
    Zone z;
};

// The inclusive element range [e_lo, e_hi] of the time array that holds every slot of the tile with ok == true (a superset),
// then lane i's load of zone e_lo / 1024 + i.  A range the arithmetic cannot vouch for — empty, past the array, wider than 64
// zones — is read and tested per row.  zones: the map of the array of n_elems elements the sweep's slot 0 reads.
template <typename FamPtr>
__device__ __forceinline__ Probe probe_tile(const SweepCommon& sw, const Zone* zones, u64 n_elems, FamPtr fams, u64 t, int lane) {
    Probe p;
    p.can = p.active = false;
    p.z = Zone{0, 0};
    const TileGeom g = tile_geom(sw, fams, t);
    u64 e_lo, e_hi;
    bool valid = g.seg_len > 0;
    if (g.form == 0) {  // dense: ordinals [j 1024, (j + 1) 1024) of the segment, cut at its end — an unaligned tile touches two zones
        const u64 o0 = g.j * kDenseTileOrdinals, o1 = o0 + kDenseTileOrdinals < g.seg_len ? o0 + kDenseTileOrdinals : g.seg_len;
        valid = valid && o0 < o1;
        e_lo = g.row_base + o0;
        e_hi = g.row_base + o1 - 1;
    } else if (g.form == 1) {  // linear: ordinals [T0, T0 + 512) cut at ord_hi, over the segments they fall into
        const u64 T0 = g.j * kTileOrdinals, last = T0 + kTileOrdinals < g.ord_hi ? T0 + kTileOrdinals : g.ord_hi;
        valid = valid && T0 < last;
        const u64 sl = valid ? g.seg_len : 1;
        const u64 seg0 = T0 / sl, seg1 = (valid ? last - 1 : 0) / sl;
        e_lo = g.col0 + seg0 * g.pitch;
        e_hi = g.col0 + seg1 * g.pitch + (g.seg_len - 1) * g.step;
    } else {  // strided: ordinals [j 512, (j + 1) 512) of the segment, cut at its end, `step` elements apart
        const u64 o0 = g.j * kTileOrdinals, o1 = o0 + kTileOrdinals < g.seg_len ? o0 + kTileOrdinals : g.seg_len;
        valid = valid && o0 < o1;
        e_lo = g.row_base + o0 * g.step;
        e_hi = g.row_base + (o1 - 1) * g.step;
    }
    e_lo = uniform64(e_lo);
    e_hi = uniform64(e_hi);
    valid = __builtin_amdgcn_readfirstlane(valid ? 1 : 0) != 0 && e_lo <= e_hi && e_hi < n_elems;
    const u64 z_lo = e_lo >> kZoneShift, z_hi = e_hi >> kZoneShift;
    p.can = valid && z_hi - z_lo < 64;
    p.active = p.can && z_lo + static_cast<u64>(lane) <= z_hi;
    if (p.active) p.z = zones[z_lo + static_cast<u64>(lane)];  // (z_hi < nzones: e_hi < n_elems)
    return p;
}

}  // namespace
}  // namespace aqe
