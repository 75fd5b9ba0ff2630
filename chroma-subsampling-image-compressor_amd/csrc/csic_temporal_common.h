// csic_temporal_common.h -- what the device codecs of the two temporal layers (csic_delta.hip, csic_mc.hip) share, on top of
// csic_pack_common.h.  Device: the kernels' argument, the checked accessors of the frames and of the maps -- a map is read and written
// as dword `dw` of `words` dwords at a byte offset, and the CSIC_DEBUG build checks dw against words and the bytes against map_bytes --,
// Host: what the entry points refuse before any device is touched and the filler of the argument (the refusals of a call are
// temporal_check_call of csic_temporal_host.h, the host codecs').  The kernels' slot loops -- price and pack the differences of a
// group against a reference group, and the add-back, both with the ragged-tail rule "slots behind the last sample: no cost, zero
// bits" -- stay written out in the units: as shared functions they cost registers or time.
#pragma once
#include "csic_pack_common.h"
#include "csic_temporal_host.h"

namespace csic {

// PkArgs: bits = the frames (the forward kernels read, the inverse kernels write); coded, ws, sizes and the coded frame's offsets are unused
struct TpArgs : PkArgs {
    uint8_t *diff;                 // difference frames, frame_bytes apart (forward writes, inverse reads)
    uint8_t *maps;                 // maps, map_stride apart
    int64_t map_stride, map_bytes;
    uint32_t moff[3], mdw[3];      // byte offset and dwords of a plane's section of the map
    int32_t nframes, gop;
};

__device__ __forceinline__ gpdst_t tp_frame(const TpArgs &a, uint8_t *first, uint32_t f) { return (gpdst_t)(uintptr_t)first + (int64_t)f * a.frame_bytes; }
__device__ __forceinline__ gpdst_t tp_map(const TpArgs &a, uint32_t f) { return (gpdst_t)(uintptr_t)a.maps + (int64_t)f * a.map_stride; }
// dword `dw` of the `words` dwords at byte `off` of a map
__device__ __forceinline__ void tp_map_word_st4(const TpArgs &a, gpdst_t mb, uint32_t off, [[maybe_unused]] uint32_t words, uint32_t dw, uint32_t v)
{
    CSIC_CHECK(dw < words);
    by_st4<false>(a.map_bytes, mb, (int64_t)off + 4 * (int64_t)dw, v);
}
__device__ __forceinline__ uint32_t tp_map_word_ld4(const TpArgs &a, gpdst_t mb, uint32_t off, [[maybe_unused]] uint32_t words, uint32_t dw)
{
    CSIC_CHECK(dw < words);
    return by_ld4<false>(a.map_bytes, mb, (int64_t)off + 4 * (int64_t)dw);
}
// dword `dw` of a plane's section of a map
__device__ __forceinline__ void tp_map_st4(const TpArgs &a, gpdst_t mb, int plane, uint32_t dw, uint32_t v) { tp_map_word_st4(a, mb, a.moff[plane], a.mdw[plane], dw, v); }
__device__ __forceinline__ uint32_t tp_map_ld4(const TpArgs &a, gpdst_t mb, int plane, uint32_t dw) { return tp_map_word_ld4(a, mb, a.moff[plane], a.mdw[plane], dw); }

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// What the device entry points of both layers refuse before any device is touched, then the geometry and the arguments filled: a
// section holds `bits` bits per group; a layer's own fields are its caller's.
template <class Geo, class Args>
int tp_prepare(csic_plan *plan, const void *d_frames, const void *d_diff, const void *d_maps, int32_t nframes, int32_t gop, int (*geometry)(const csic_params *, Geo *),
               bool in_place_ok, int bits, const char *entry, Geo *G, Args *a)
{
    if (!plan) return set_error(CSIC_EINVAL_NULL, "plan is NULL");
    if (!d_frames || !d_diff || !d_maps) return set_error(CSIC_EINVAL_NULL, "device buffer is NULL");
    int st = geometry(&plan->p, G);
    if (st == CSIC_OK) st = temporal_check_call(*G, d_frames, d_diff, d_maps, nframes, gop, in_place_ok);
    if (st != CSIC_OK) return st;
    if (((uintptr_t)d_frames | (uintptr_t)d_diff | (uintptr_t)d_maps) & 255u)
        return set_error(CSIC_EINVAL_SIZE, "the frames, the difference frames and the maps must be 256-byte aligned");
    const int64_t none[3] = {0, 0, 0};
    st = pk_fill_args(plan, G->pk, none, none, 0, 0, entry, a);
    if (st != CSIC_OK) return st;
    a->bits = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_frames));
    a->diff = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_diff));
    a->maps = const_cast<uint8_t *>(static_cast<const uint8_t *>(d_maps));
    a->map_stride = G->layout.map_stride;
    a->map_bytes = G->layout.map_bytes;
    for (int p = 0; p < 3; ++p) {
        a->moff[p] = (uint32_t)G->layout.map_offset[p];
        a->mdw[p] = (uint32_t)((G->layout.groups[p] * bits + 31) / 32);
    }
    a->nframes = nframes;
    a->gop = gop > nframes ? nframes : gop;                                 // (a run never passes the last frame: z gop + gop stays small)
    return CSIC_OK;
}

} // namespace csic
