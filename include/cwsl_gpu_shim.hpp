// cwsl_gpu_shim.hpp -- header-only C++17 shim that turns the C ABI of libcwslgpu.so back into the shapes
// the reference's call sites use, so Receiver / Instance / DecoderPool code compiles against the GPU path
// with one-line changes.
//
//   cwslgpu::Context          process-wide handle (one per GPU)
//   cwslgpu::ReceiverPort     what Receiver::readIQ writes into instead of ring_buffer_spmc_t
//                             (source/Receiver.hpp:247-249)
//   cwslgpu::SsbChannel       SSBD<float>-shaped object: same constructor arguments, same getters (GetInRate, GetOutRate,
//                             GetInSize, GetOutSize, GetBandwidth, GetCarrier, IsUSB, GetDelay: source/SSBD.hpp:140-154),
//                             same Tune, same std::invalid_argument messages (source/SSBD.hpp:48-59,97-103)
//   cwslgpu::FrameSink        what Instance::sampleManager does after a slot boundary (source/Instance.cpp:221-245) for a
//                             set of channels: every newly finalised frame goes to a callback as the ingredients of
//                             ItemToDecode (DecoderPool.hpp:174-210)
//
// SSBD::Iterate(in, out) (SSBD.hpp:127-137) is deliberately absent: its contract is a synchronous 64-samples-in / 4-samples-out
// call, which on a GPU is one kernel launch and one device-to-host wait per 4 output samples; its only caller in the reference
// is the loop of Instance::sampleManager (Instance.cpp:273) that ReceiverPort::push + Context::slotBoundary + SsbChannel::fetch
// replace as a whole.
//
// Nothing here computes DSP: every call forwards to the C ABI.
#pragma once
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include <array>
#include <algorithm>
#include <cstring>
#include <complex>

#include "cwsl_gpu.h"

namespace cwslgpu {

inline void check(cwslg_ctx *c, int rc)
{
    if (rc >= 0) return;
    const char *detail = c ? cwslg_last_error(c) : "";
    std::string msg = (detail && *detail) ? detail : cwslg_strerror(rc);
    // the reference throws std::invalid_argument for the three tuning errors (SSBD.hpp:54-59,100-103)
    if (rc == CWSLG_ERR_RATIO || rc == CWSLG_ERR_BAND_LOW || rc == CWSLG_ERR_BAND_HIGH)
        throw std::invalid_argument(cwslg_strerror(rc));
    if (rc == CWSLG_ERR_MODE) throw std::runtime_error(msg);          // CWSL_DIGI.hpp:111
    throw std::runtime_error("libcwslgpu: " + msg);
}

// What cwslg_fetch_ft8_ap and cwslg_fetch_ft4_ap leave to the host: `decodes` (cwslg_fetch_decodes) followed by those records of `ap` (the
// a-priori call of the same group and epoch) whose bits[12] no record of `decodes` with the same ch_id carries -- BP / OSD win -- in ascending (ch_id, entry, by_osd).
inline std::vector<cwslg_decode> mergeApDecodes(const std::vector<cwslg_decode> &decodes, const std::vector<cwslg_decode> &ap)
{
    std::vector<cwslg_decode> out(decodes);
    for (const cwslg_decode &a : ap) {
        bool have = false;
        for (const cwslg_decode &d : decodes)
            if (d.ch_id == a.ch_id && std::memcmp(d.bits, a.bits, sizeof(a.bits)) == 0) { have = true; break; }
        if (!have) out.push_back(a);
    }
    std::stable_sort(out.begin(), out.end(), [](const cwslg_decode &x, const cwslg_decode &y) {
        if (x.ch_id != y.ch_id) return x.ch_id < y.ch_id;
        if (x.entry != y.entry) return x.entry < y.entry;
        return x.by_osd < y.by_osd;
    });
    return out;
}

// The `set` byte of an FT4 a-priori record (cwslg_fetch_ft4_ap: by_osd = 2) -> {metric set, pattern index}
inline std::array<int, 2> apSetSplit(std::uint8_t set)
{
    return {set & 3, set >> 2};
}

// Which of a cwslg_ft4_msg's three sets a consumer takes: upstream tries the metric sets in order and stops at the first success, which is the
// smallest s with crc_ok; -1 if none has it
inline int ft4BestSet(const cwslg_ft4_msg &m)
{
    for (int s = 0; s < 3; ++s)
        if (m.set[s].crc_ok) return s;
    return -1;
}

// Which word a consumer takes from a record's cwslg_ft4_msg and cwslg_ft4_osd: the smallest s with BP crc_ok (ft4BestSet); if there is none, the
// smallest s with OSD crc_ok, *byOsd = true (take osd.set[s].bits then, not msg.set[s].bits); -1 if neither stage has a word
inline int ft4BestWord(const cwslg_ft4_msg &m, const cwslg_ft4_osd &o, bool *byOsd = nullptr)
{
    if (byOsd) *byOsd = false;
    const int s = ft4BestSet(m);
    if (s >= 0) return s;
    for (int k = 0; k < 3; ++k)
        if (o.set[k].crc_ok) {
            if (byOsd) *byOsd = true;
            return k;
        }
    return -1;
}

class Context {
public:
    explicit Context(int device = -1) { check(nullptr, cwslg_create(&c_, device)); }
    ~Context() { cwslg_destroy(c_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    cwslg_ctx *raw() const { return c_; }
    void setScaleFactors(float ft, float wspr) { check(c_, cwslg_set_scale_factors(c_, ft, wspr)); }
    // SyncPredicate::store(true) for a whole group (CWSL_DIGI.cpp:247-251)
    void slotBoundary(int group, std::uint64_t epoch_s) { check(c_, cwslg_slot_boundary(c_, group, epoch_s)); }
    void process() { check(c_, cwslg_process(c_)); }
    // soft bits per FT8 sync candidate from the next boundary on (needs the sync stage: cwslg_enable_sync) -- SsbChannel::fetchFt8Softbits
    void enableFt8Softbits(bool enable = true) { check(c_, cwslg_enable_ft8_softbits(c_, enable ? 1 : 0)); }
    // soft bits per refined FT4 sync record from the next boundary on (needs the sync stage; records only while the coherent stage runs) -- SsbChannel::fetchFt4Softbits
    void enableFt4Softbits(bool enable = true) { check(c_, cwslg_enable_ft4_softbits(c_, enable ? 1 : 0)); }
    // FT8 decode: the (174, 91) parity-check table is the caller's data -- nm[83 * 7], the Nm table of the integrator's own WSJT-X tree
    // (cwslg_set_ldpc_code validates it); then LDPC decode + CRC-14 per FT8 sync candidate from the next boundary on (needs a loaded code, the sync
    // stage and FT8 soft bits) -- SsbChannel::fetchFt8Decode; ldpcDecode runs the same kernel on caller-supplied metrics (the FT4 path)
    void setLdpcCode(const std::uint8_t *nm) { check(c_, cwslg_set_ldpc_code(c_, nm)); }
    void enableFt8Decode(bool enable = true, int maxIter = 30, int minNsync = 7) { check(c_, cwslg_enable_ft8_decode(c_, enable ? 1 : 0, maxIter, minNsync)); }
    void ldpcDecode(const float *llr, int n, std::vector<cwslg_ft8_msg> &out, int maxIter = 30)
    {
        out.resize(n);
        check(c_, cwslg_ldpc_decode(c_, llr, n, maxIter, out.data()));
    }
    // FT4 decode: the same decode on the three metric sets of every FT4 soft-bit record from the next boundary on (needs a loaded code, the sync
    // stage and FT4 soft bits; records only while the coherent stage runs) -- SsbChannel::fetchFt4Decode, ft4BestSet
    void enableFt4Decode(bool enable = true, int maxIter = 30, int minNsync = 8, int minNqual = 20)
    {
        check(c_, cwslg_enable_ft4_decode(c_, enable ? 1 : 0, maxIter, minNsync, minNqual));
    }
    // FT4 OSD: the same OSD on the metric sets of the FT4 records no set of which the decode brought to crc_ok, from the next boundary at which
    // the coherent stage, soft bits and decode are on too (needs a loaded code of rank 83) -- SsbChannel::fetchFt4Osd, ft4BestWord
    void enableFt4Osd(bool enable = true, int order = 2, int minNsync = 8, int minNqual = 20)
    {
        check(c_, cwslg_enable_ft4_osd(c_, enable ? 1 : 0, order, minNsync, minNqual));
    }
    // FT8 OSD: ordered-statistics decoding (order 0..2) of the candidates the decode attempted without crc_ok, from the next boundary at which
    // soft bits and decode are on too (needs a loaded code of rank 83) -- SsbChannel::fetchFt8Osd; osdDecode runs the same kernel on
    // caller-supplied metrics
    void enableFt8Osd(bool enable = true, int order = 2, int minNsync = 7) { check(c_, cwslg_enable_ft8_osd(c_, enable ? 1 : 0, order, minNsync)); }
    void osdDecode(const float *llr, int n, std::vector<cwslg_osd_msg> &out, int order = 2)
    {
        out.resize(n);
        check(c_, cwslg_osd_decode(c_, llr, n, order, out.data()));
    }
    // The decodes of a slot: the words of a whole FT8 / FT4 slot-clock group in one fetch, chosen (BP before OSD) and de-duplicated per channel on
    // the device (cwslg_fetch_decodes).  startEpoch in / out: 0 asks for the newest epoch any channel of the group has decode records of.  `out`
    // gets the first min(total, max) decodes in ascending (ch_id, entry); the return value is the total; 0 with `out` empty and startEpoch
    // untouched while no channel takes part.  nChannels (optional): channels that took part.
    int fetchDecodes(int group, std::vector<cwslg_decode> &out, std::uint64_t &startEpoch, int max = 4096, int *nChannels = nullptr)
    {
        out.resize(max > 0 ? max : 0);
        int n = 0, total = 0;
        const int rc = cwslg_fetch_decodes(c_, group, &startEpoch, out.data(), static_cast<int>(out.size()), &n, &total, nChannels);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); return 0; }
        check(c_, rc);
        out.resize(n);
        return total;
    }
    // The same fetch with a signal report per decode (cwslg_fetch_decode_reports; FT8 group only): reports[p] belongs to out[p] -- snr_db for the
    // spot, nsync / nsymerr to gate on.  Needs a systematic code loaded (cwslg_set_ldpc_code); the words are re-encoded under the code in force.
    int fetchDecodeReports(int group, std::vector<cwslg_decode> &out, std::vector<cwslg_decode_report> &reports, std::uint64_t &startEpoch, int max = 4096,
                           int *nChannels = nullptr)
    {
        out.resize(max > 0 ? max : 0);
        reports.resize(out.size());
        int n = 0, total = 0;
        const int rc = cwslg_fetch_decode_reports(c_, group, &startEpoch, out.data(), reports.data(), static_cast<int>(out.size()), &n, &total, nChannels);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); reports.clear(); return 0; }
        check(c_, rc);
        out.resize(n);
        reports.resize(n);
        return total;
    }
    // FT8 signal subtraction (cwslg_subtract_ft8): fetchDecodes("FT8") with a refined fit per decode -- sub[p].f_hz / dt_s are what to report
    // instead of out[p]'s grid values -- and a residual frame per channel left on the device: ft8Residual copies it (180000 floats, the units of
    // the float frame), ft8ResidualDevice hands out its address; both return false once the channel's frame is of another epoch.  Needs a
    // systematic code loaded.  ft8SubtractFlat: the same kernels on frames and items of the caller's own.
    int subtractFt8(std::vector<cwslg_decode> &out, std::vector<cwslg_subtract_report> &sub, std::uint64_t &startEpoch, int max = 4096, int *nChannels = nullptr)
    {
        out.resize(max > 0 ? max : 0);
        sub.resize(out.size());
        int n = 0, total = 0;
        const int rc = cwslg_subtract_ft8(c_, &startEpoch, out.data(), sub.data(), static_cast<int>(out.size()), &n, &total, nChannels);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); sub.clear(); return 0; }
        check(c_, rc);
        out.resize(n);
        sub.resize(n);
        return total;
    }
    bool ft8Residual(int chId, std::vector<float> &out, std::uint64_t *startEpoch = nullptr)
    {
        out.resize(CWSLG_FT8_FRAME_SAMPLES);
        const int rc = cwslg_fetch_ft8_residual(c_, chId, out.data(), out.size(), nullptr, startEpoch);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); return false; }
        check(c_, rc);
        return true;
    }
    bool ft8ResidualDevice(int chId, const float *&dF32, std::uint64_t *startEpoch = nullptr)
    {
        const int rc = cwslg_ft8_residual_device_ptr(c_, chId, &dF32, startEpoch);
        if (rc == CWSLG_ERR_NO_FRAME) return false;
        check(c_, rc);
        return true;
    }
    void ft8SubtractFlat(const float *audio, int nFrames, const std::vector<cwslg_ft8_sub_item> &items, std::vector<cwslg_subtract_report> &sub,
                         std::vector<float> *residual = nullptr)
    {
        sub.resize(items.size());
        if (residual) residual->resize(static_cast<std::size_t>(nFrames > 0 ? nFrames : 0) * CWSLG_FT8_FRAME_SAMPLES);
        check(c_, cwslg_ft8_subtract_flat(c_, audio, nFrames, items.empty() ? nullptr : items.data(), static_cast<int>(items.size()),
                                          sub.empty() ? nullptr : sub.data(), residual ? residual->data() : nullptr));
    }
    // FT4 signal subtraction (cwslg_subtract_ft4): the same for the FT4 group -- fetchDecodes("FT4") with a refined fit per decode and a residual
    // of 72576 floats per FT4 channel (ft4Residual, ft4ResidualDevice; false for an FT8 channel's id).  ft4SubtractFlat: frames of 72576 floats.
    int subtractFt4(std::vector<cwslg_decode> &out, std::vector<cwslg_subtract_report> &sub, std::uint64_t &startEpoch, int max = 4096, int *nChannels = nullptr)
    {
        out.resize(max > 0 ? max : 0);
        sub.resize(out.size());
        int n = 0, total = 0;
        const int rc = cwslg_subtract_ft4(c_, &startEpoch, out.data(), sub.data(), static_cast<int>(out.size()), &n, &total, nChannels);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); sub.clear(); return 0; }
        check(c_, rc);
        out.resize(n);
        sub.resize(n);
        return total;
    }
    bool ft4Residual(int chId, std::vector<float> &out, std::uint64_t *startEpoch = nullptr)
    {
        out.resize(CWSLG_FT4_FRAME_SAMPLES);
        const int rc = cwslg_fetch_ft4_residual(c_, chId, out.data(), out.size(), nullptr, startEpoch);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); return false; }
        check(c_, rc);
        return true;
    }
    bool ft4ResidualDevice(int chId, const float *&dF32, std::uint64_t *startEpoch = nullptr)
    {
        const int rc = cwslg_ft4_residual_device_ptr(c_, chId, &dF32, startEpoch);
        if (rc == CWSLG_ERR_NO_FRAME) return false;
        check(c_, rc);
        return true;
    }
    void ft4SubtractFlat(const float *audio, int nFrames, const std::vector<cwslg_ft4_sub_item> &items, std::vector<cwslg_subtract_report> &sub,
                         std::vector<float> *residual = nullptr)
    {
        sub.resize(items.size());
        if (residual) residual->resize(static_cast<std::size_t>(nFrames > 0 ? nFrames : 0) * CWSLG_FT4_FRAME_SAMPLES);
        check(c_, cwslg_ft4_subtract_flat(c_, audio, nFrames, items.empty() ? nullptr : items.data(), static_cast<int>(items.size()),
                                          sub.empty() ? nullptr : sub.data(), residual ? residual->data() : nullptr));
    }
    // FT8 a-priori decoding: the patterns are the caller's data (cwslg_set_ft8_ap validates them: at most 8, none clears them), tried in this
    // order on the candidates BP and OSD gave up on.  apDecode runs the kernel on caller-supplied metrics; fetchFt8Ap is fetchDecodes' shape for
    // the a-priori words of the FT8 group (by_osd = 2, set = the pattern, dmin = OSD's distance of the word): words BP / OSD already have are
    // not removed there -- mergeApDecodes below.
    void setFt8Ap(const cwslg_ap_pattern *patterns, int nPatterns, int maxIter = 30, int minNsync = 7)
    {
        check(c_, cwslg_set_ft8_ap(c_, patterns, nPatterns, maxIter, minNsync));
    }
    void setFt8Ap(const std::vector<cwslg_ap_pattern> &patterns, int maxIter = 30, int minNsync = 7)
    {
        setFt8Ap(patterns.empty() ? nullptr : patterns.data(), static_cast<int>(patterns.size()), maxIter, minNsync);
    }
    void apDecode(const float *llr, int n, std::vector<cwslg_ap_msg> &out)
    {
        out.resize(n);
        check(c_, cwslg_ap_decode(c_, llr, n, out.data()));
    }
    int fetchFt8Ap(std::vector<cwslg_decode> &out, std::uint64_t &startEpoch, int max = 4096, int *nChannels = nullptr)
    {
        out.resize(max > 0 ? max : 0);
        int n = 0, total = 0;
        const int rc = cwslg_fetch_ft8_ap(c_, &startEpoch, out.data(), static_cast<int>(out.size()), &n, &total, nChannels);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); return 0; }
        check(c_, rc);
        out.resize(n);
        return total;
    }
    // FT4 a-priori decoding: patterns of their own beside the FT8 ones (FT4's message bits are scrambled on the air, so the values differ), the
    // FT4 decode's two minima; fetchFt4Ap is fetchFt8Ap for the FT4 group, with set = metric set | pattern << 2 (apSetSplit).
    void setFt4Ap(const cwslg_ap_pattern *patterns, int nPatterns, int maxIter = 30, int minNsync = 8, int minNqual = 20)
    {
        check(c_, cwslg_set_ft4_ap(c_, patterns, nPatterns, maxIter, minNsync, minNqual));
    }
    void setFt4Ap(const std::vector<cwslg_ap_pattern> &patterns, int maxIter = 30, int minNsync = 8, int minNqual = 20)
    {
        setFt4Ap(patterns.empty() ? nullptr : patterns.data(), static_cast<int>(patterns.size()), maxIter, minNsync, minNqual);
    }
    int fetchFt4Ap(std::vector<cwslg_decode> &out, std::uint64_t &startEpoch, int max = 4096, int *nChannels = nullptr)
    {
        out.resize(max > 0 ? max : 0);
        int n = 0, total = 0;
        const int rc = cwslg_fetch_ft4_ap(c_, &startEpoch, out.data(), static_cast<int>(out.size()), &n, &total, nChannels);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); return 0; }
        check(c_, rc);
        out.resize(n);
        return total;
    }
    // The 79 channel tones of a 91-bit word (cwslg_decode.bits) under the code in force: the reports' re-encoder on its own, host work only
    std::array<std::uint8_t, 79> ft8Tones(const std::uint8_t *bits12)
    {
        std::array<std::uint8_t, 79> t{};
        check(c_, cwslg_ft8_tones(c_, bits12, t.data()));
        return t;
    }
    // The FT4 group's fetch with a signal report per decode (cwslg_fetch_ft4_decode_reports): reports[p] belongs to out[p]; nsync is 0..16, nsymerr
    // 0..87, snr_db never below -21.  Needs a systematic code loaded; the words are re-encoded under the code in force (no rvec).
    int fetchFt4DecodeReports(std::vector<cwslg_decode> &out, std::vector<cwslg_decode_report> &reports, std::uint64_t &startEpoch, int max = 4096,
                              int *nChannels = nullptr)
    {
        out.resize(max > 0 ? max : 0);
        reports.resize(out.size());
        int n = 0, total = 0;
        const int rc = cwslg_fetch_ft4_decode_reports(c_, &startEpoch, out.data(), reports.data(), static_cast<int>(out.size()), &n, &total, nChannels);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); reports.clear(); return 0; }
        check(c_, rc);
        out.resize(n);
        reports.resize(n);
        return total;
    }
    // The 103 FT4 channel tones of a 91-bit word (cwslg_decode.bits) under the code in force: host work only
    std::array<std::uint8_t, 103> ft4Tones(const std::uint8_t *bits12)
    {
        std::array<std::uint8_t, 103> t{};
        check(c_, cwslg_ft4_tones(c_, bits12, t.data()));
        return t;
    }
    void synchronize() { check(c_, cwslg_synchronize(c_)); }
    // One block for each of several receivers in ONE call (cwslg_push_iq_many): for a host that serves thousands of streams, where a
    // per-receiver push per block (Receiver.hpp:242-249, ReceiverPort::push below) would mean hundreds of thousands of copies a second.
    // ids[k] = ReceiverPort::id(); blocks[k] = that receiver's n_complex samples.
    void pushMany(const std::vector<int> &ids, const std::vector<const std::complex<float> *> &blocks, std::uint32_t n_complex)
    {
        if (ids.size() != blocks.size()) throw std::invalid_argument("pushMany: one block per receiver");
        check(c_, cwslg_push_iq_many(c_, static_cast<int>(ids.size()), ids.data(), reinterpret_cast<const float *const *>(blocks.data()), n_complex));
    }
private:
    cwslg_ctx *c_ = nullptr;
};

// Receiver side: `memcpy(iq_buffer.recs[write_index], rawiq.data(), readSize); iq_buffer.inc_write_index();`
// becomes `port.push(rawiq.data(), iq_len);`
class ReceiverPort {
public:
    ReceiverPort(Context &ctx, std::uint32_t sampleRate, std::uint32_t blockInSamples, std::int32_t lo_hz,
                 std::uint32_t ringBlocks = 0) : ctx_(ctx), fs_(sampleRate)
    {
        check(ctx_.raw(), cwslg_receiver_open(ctx_.raw(), sampleRate, blockInSamples, lo_hz, ringBlocks, &id_));
    }
    ~ReceiverPort() { cwslg_receiver_close(ctx_.raw(), id_); }
    void push(const std::complex<float> *block, std::uint32_t n_complex)
    {
        check(ctx_.raw(), cwslg_push_iq(ctx_.raw(), id_, reinterpret_cast<const float *>(block), n_complex));
    }
    int id() const { return id_; }
    std::uint32_t sampleRate() const { return fs_; }     // Receiver::getSampleRate
    Context &context() const { return ctx_; }
private:
    Context &ctx_;
    int id_ = -1;
    std::uint32_t fs_ = 0;
};

// SSBD<float>(Fs, B, F, isUSB) -> SsbChannel(port, F, isUSB, mode).  Fs comes from the port; B is SSB_BW.
// F is a whole number of Hz: the reference passes static_cast<float>(demodFreq) of an integer FrequencyHz (Instance.cpp:183-187,
// 251), the C ABI takes it as int32 -- a fractional F given here is truncated toward zero, not rounded.
class SsbChannel {
public:
    SsbChannel(ReceiverPort &port, double F, bool isUSB, const std::string &mode)
        : ctx_(port.context()), mode_(mode), fs_(port.sampleRate()), carrier_(static_cast<double>(static_cast<std::int32_t>(F))), usb_(isUSB)
    {
        check(ctx_.raw(), cwslg_channel_open(ctx_.raw(), port.id(), static_cast<std::int32_t>(F), isUSB ? 1 : 0,
                                             mode.c_str(), &id_));
        check(ctx_.raw(), cwslg_channel_info(ctx_.raw(), id_, &in_, &out_, &rate_, &delay_, &frame_));
    }
    ~SsbChannel() { cwslg_channel_close(ctx_.raw(), id_); }
    std::size_t GetInRate() const { return fs_; }       // SSBD.hpp:140
    std::size_t GetOutRate() const { return rate_; }    // :142
    std::size_t GetInSize() const { return in_; }       // :144
    std::size_t GetOutSize() const { return out_; }     // :146
    std::size_t GetBandwidth() const { return rate_ / 2; }   // :148  (GetOutRate() is 2*B)
    double GetCarrier() const { return carrier_; }      // :150  the tuned frequency F as last set (constructor or Tune)
    bool IsUSB() const { return usb_; }                 // :152
    std::size_t GetDelay() const { return delay_; }     // :154
    const std::string &mode() const { return mode_; }
    float trPeriod() const { return static_cast<float>(frame_ / 12000) - 5.0f; }    // frame = 12000 * (period + 5), Instance.cpp:149
    // SSBD::Tune(F, isUSB, reset = true) (SSBD.hpp:97): throws the same std::invalid_argument texts; the old tuning stays in force
    // after a throw.  reset = false keeps filter history, block position and phase, as :116-121 does when skipped.
    void Tune(double F, bool isUSB, bool reset = true)
    {
        const int rc = cwslg_channel_tune_ex(ctx_.raw(), id_, static_cast<std::int32_t>(F), isUSB ? 1 : 0, reset ? 1 : 0);
        if (rc == CWSLG_ERR_BAND_LOW || rc == CWSLG_ERR_BAND_HIGH || rc == CWSLG_ERR_RATIO) throw std::invalid_argument(cwslg_strerror(rc));
        check(ctx_.raw(), rc);
        carrier_ = static_cast<double>(static_cast<std::int32_t>(F));
        usb_ = isUSB;
    }
    std::size_t frameLength() const { return frame_; }  // Instance.cpp:149
    int id() const { return id_; }

    // What Instance.cpp:238-245 hands to DecoderPool::push: returns false while no frame is ready
    // (first partial slot).  audio is resized to frameLength().
    bool fetch(std::vector<std::int16_t> &audio, std::uint64_t &startEpoch)
    {
        audio.resize(frame_);
        std::size_t nv = 0;
        const int rc = cwslg_fetch_frame(ctx_.raw(), id_, audio.data(), audio.size(), &startEpoch, &nv, nullptr);
        if (rc == CWSLG_ERR_NO_FRAME) return false;
        check(ctx_.raw(), rc);
        return true;
    }
    // startEpoch (optional): the start epoch of the frame the list was computed from -- pair it with fetch()'s, or use fetchSlot()
    int candidates(std::vector<cwslg_candidate> &out, int max = 600, std::uint64_t *startEpoch = nullptr)
    {
        out.resize(max);
        int n = 0;
        check(ctx_.raw(), cwslg_fetch_candidates(ctx_.raw(), id_, out.data(), max, &n, startEpoch));
        out.resize(n);
        return n;
    }
    // The ItemToDecode of one slot (DecoderPool.hpp:174-210: audio + epochTime travel together) with the candidate list of the SAME epoch,
    // in one call and under one ticket (cwslg_fetch_slot): false while no frame is ready.  FT8 / FT4 channels.
    bool fetchSlot(std::vector<std::int16_t> &audio, std::uint64_t &startEpoch, std::vector<cwslg_candidate> &cands, int max = 600)
    {
        audio.resize(frame_);
        cands.resize(max);
        cwslg_slot_result r;
        const int rc = cwslg_fetch_slot(ctx_.raw(), id_, audio.data(), audio.size(), cands.data(), cands.size() * sizeof(cwslg_candidate),
                                        nullptr, 0, &r);
        if (rc == CWSLG_ERR_NO_FRAME) { cands.clear(); return false; }
        check(ctx_.raw(), rc);
        startEpoch = r.start_epoch;
        cands.resize((r.list_kind == CWSLG_LIST_FT8 || r.list_kind == CWSLG_LIST_FT4) ? r.n_list : 0);
        return true;
    }
    // FT4 channels: every candidate refined coherently (start sample, frequency tweak, sync) -- cwslg_fetch_ft4_sync
    int ft4Sync(std::vector<cwslg_ft4_sync> &out, int max = 1800)
    { return fetchRecords(cwslg_fetch_ft4_sync, out, max, nullptr); }
    // FT8 channels with Context::enableFt8Softbits: record q (174 bit metrics, sigma, nsync) belongs to entry q of candidates() of the same
    // epoch -- cwslg_fetch_ft8_softbits; 0 records while none of the current epoch exist
    int fetchFt8Softbits(std::vector<cwslg_ft8_soft> &out, int max = 600, std::uint64_t *startEpoch = nullptr)
    { return fetchRecords(cwslg_fetch_ft8_softbits, out, max, startEpoch); }
    // FT8 channels with Context::enableFt8Decode: record q (91 bits, iters, nbad, nharderr, crc_ok) belongs to entry q of candidates() of the same
    // epoch -- cwslg_fetch_ft8_decode; 0 records while none of the current epoch exist
    int fetchFt8Decode(std::vector<cwslg_ft8_msg> &out, int max = 600, std::uint64_t *startEpoch = nullptr)
    { return fetchRecords(cwslg_fetch_ft8_decode, out, max, startEpoch); }
    // FT4 channels with Context::enableFt4Decode: record q (three cwslg_ft8_msg, one per metric set) belongs to entry q of cwslg_fetch_ft4_sync of
    // the same epoch -- cwslg_fetch_ft4_decode; 0 records while none of the current epoch exist
    int fetchFt4Decode(std::vector<cwslg_ft4_msg> &out, int max = 1800, std::uint64_t *startEpoch = nullptr)
    { return fetchRecords(cwslg_fetch_ft4_decode, out, max, startEpoch); }
    // FT4 channels with Context::enableFt4Osd: record q (three cwslg_osd_msg, one per metric set) belongs to entry q of cwslg_fetch_ft4_sync of
    // the same epoch -- cwslg_fetch_ft4_osd; 0 records while none of the current epoch exist
    int fetchFt4Osd(std::vector<cwslg_ft4_osd> &out, int max = 1800, std::uint64_t *startEpoch = nullptr)
    { return fetchRecords(cwslg_fetch_ft4_osd, out, max, startEpoch); }
    // FT8 channels with Context::enableFt8Osd: record q (91 bits, dmin, nharderr, nskip, crc_ok, how, flip) belongs to entry q of candidates() of
    // the same epoch -- cwslg_fetch_ft8_osd; 0 records while none of the current epoch exist
    int fetchFt8Osd(std::vector<cwslg_osd_msg> &out, int max = 600, std::uint64_t *startEpoch = nullptr)
    { return fetchRecords(cwslg_fetch_ft8_osd, out, max, startEpoch); }
    // FT4 channels with Context::enableFt4Softbits: record q (three sets of 174 bit metrics, their sigma, nsync, nqual) belongs to entry q of
    // cwslg_fetch_ft4_sync of the same epoch -- cwslg_fetch_ft4_softbits; 0 records while none of the current epoch exist
    int fetchFt4Softbits(std::vector<cwslg_ft4_soft> &out, int max = 1800, std::uint64_t *startEpoch = nullptr)
    { return fetchRecords(cwslg_fetch_ft4_softbits, out, max, startEpoch); }
    // what decodeUsingShMem does between lock and unlock (DecoderPool.hpp:451-590): the jt9 block, d2 straight from HBM
    bool fillDecoderBlock(void *block, std::size_t bytes, int decodedepth, int highestDecodeFreq, std::uint64_t &startEpoch, bool js8 = false)
    {
        const int rc = cwslg_fill_decoder_block(ctx_.raw(), id_, block, bytes, js8 ? 1 : 0, decodedepth, highestDecodeFreq, &startEpoch);
        if (rc == CWSLG_ERR_NO_FRAME) return false;
        check(ctx_.raw(), rc);
        return true;
    }
private:
    // one record fetch of the C ABI into `out`, sized to what came back: the number of records, 0 (and `out` empty) while there are none to fetch
    template <class Rec, class Fetch> int fetchRecords(Fetch fetch, std::vector<Rec> &out, int max, std::uint64_t *startEpoch)
    {
        out.resize(max);
        int n = 0;
        const int rc = fetch(ctx_.raw(), id_, out.data(), max, &n, startEpoch);
        if (rc == CWSLG_ERR_NO_FRAME) { out.clear(); return 0; }
        check(ctx_.raw(), rc);
        out.resize(n);
        return n;
    }
    Context &ctx_;
    int id_ = -1;
    std::string mode_;
    std::uint32_t fs_ = 0;
    double carrier_ = 0.0;
    bool usb_ = true;
    std::uint32_t in_ = 0, out_ = 0, rate_ = 0, delay_ = 0;
    std::size_t frame_ = 0;
};

// What Instance::sampleManager does with a finished frame (Instance.cpp:221-245), for every channel registered here:
//     ItemToDecode toDecode(audioBuf_i16, digitalMode, startTime, ssbFreq, static_cast<int>(id), cwd, trperiod);
//     decoderPool->push(toDecode);
// Call collect() after Context::slotBoundary(): each channel whose last finalised frame is new (its startEpochTime differs from the one
// delivered before; the first, discarded slot yields none, :224-227) is fetched and handed to the callback with those arguments.
class FrameSink {
public:
    using Callback = std::function<void(std::vector<std::int16_t> &&audio, const std::string &mode, std::uint64_t epochTime,
                                        std::int64_t baseFreq, int instanceId, const std::string &cwd, float trperiod)>;
    // ABI 5: the same hand-off with the candidate list of the SAME epoch beside the audio (cwslg_fetch_slot: one call, one ticket) -- for a decoder
    // pool whose ItemToDecode (DecoderPool.hpp:174-210) is extended by a candidate vector; FT8 / FT4 channels with the sync stage on, empty otherwise
    using SlotCallback = std::function<void(std::vector<std::int16_t> &&audio, const std::string &mode, std::uint64_t epochTime,
                                            std::int64_t baseFreq, int instanceId, const std::string &cwd, float trperiod,
                                            std::vector<cwslg_candidate> &&candidates)>;
    explicit FrameSink(Callback cb) : cb_(std::move(cb)) {}
    explicit FrameSink(SlotCallback cb, int maxCandidates = 600) : scb_(std::move(cb)), max_cand_(maxCandidates) {}
    // ssbFreq, instanceId, cwd: Instance's members of the same names (Instance.cpp:121-176)
    void add(SsbChannel &ch, std::int64_t ssbFreq, int instanceId, const std::string &cwd)
    {
        entries_.push_back(Entry{&ch, ssbFreq, instanceId, cwd, 0, false});
    }
    // returns the number of frames delivered
    int collect()
    {
        int n = 0;
        for (Entry &e : entries_) {
            std::vector<std::int16_t> audio;
            std::vector<cwslg_candidate> cands;
            std::uint64_t t0 = 0;
            if (!(scb_ ? e.ch->fetchSlot(audio, t0, cands, max_cand_) : e.ch->fetch(audio, t0))) continue;
            if (e.seen && t0 == e.last) continue;            // that frame went out at an earlier boundary
            e.seen = true;
            e.last = t0;
            if (scb_) scb_(std::move(audio), e.ch->mode(), t0, e.ssbFreq, e.instanceId, e.cwd, e.ch->trPeriod(), std::move(cands));
            else cb_(std::move(audio), e.ch->mode(), t0, e.ssbFreq, e.instanceId, e.cwd, e.ch->trPeriod());
            ++n;
        }
        return n;
    }
private:
    struct Entry { SsbChannel *ch; std::int64_t ssbFreq; int instanceId; std::string cwd; std::uint64_t last; bool seen; };
    Callback cb_;
    SlotCallback scb_;
    int max_cand_ = 600;
    std::vector<Entry> entries_;
};

} // namespace cwslgpu
