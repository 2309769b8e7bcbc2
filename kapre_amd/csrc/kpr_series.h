// kpr_series.h -- the series vocabulary of the waveform kernels (k_yin, k_cqt, k_resample, k_resample_direct, k_lfilter): how one
// series of a (batch, channels, time) batch is addressed in either layout, and which series a workgroup owns.
// Part of the single translation unit kapre_hip.hip (right after kpr_cols.h).
//
// A series is the samples of one (batch item, channel).  Three strides address it, in elements: `item` from one batch item to the
// next, `chan` from one channel of an item to the next, `stride` from one sample to the next -- channels_first (C T, T, 1),
// channels_last (C T, 1, C); series_of (kpr_host.h) fills them.  The argument structs carry them as flat fields of these names
// (out_* for an output of another length), in each struct's own order.  Workgroups are numbered series-major:
// blockIdx.x = (item n + channel) units + unit, `units` work units per series (frame runs, tiles, segments), n channels per item.
// (k_lfilter shares the fields and the numbering and decodes it in its own lines, after its early return.)
#pragma once

namespace kpr {

struct Series {
    long long item, chan;
    int stride;
};

// the series s = item n + ch and the work unit of this workgroup
struct SeriesUnit {
    int s, unit, n;
    KPR_DEV int item() const { return s / n; }
    KPR_DEV int ch() const { return s - item() * n; }
    // the series' first element: as an offset, and as a pointer from the tensor's base
    KPR_DEV long long off(long long item_stride, long long chan_stride) const { return item() * item_stride + ch() * chan_stride; }
    template <class T>
    KPR_DEV T* at(T* base, long long item_stride, long long chan_stride) const { return base + item() * item_stride + ch() * chan_stride; }
};
KPR_DEV SeriesUnit series_unit(int units, int n) {
    SeriesUnit u;
    u.s = blockIdx.x / units;
    u.unit = blockIdx.x - u.s * units;
    u.n = n;
    return u;
}

// a run of F consecutive frames of a series: its first frame, and how many of the series' frames it holds
struct FrameRun {
    int t0, fv;
};
KPR_DEV FrameRun frame_run(int run, int F, int frames) {
    FrameRun r;
    r.t0 = run * F;
    r.fv = min(F, frames - r.t0);
    return r;
}

}  // namespace kpr
