// mailbox_host.hpp — host only: the single-env mailbox.  An OcMailbox is 4 KiB of pinned, GPU-mapped host memory and one resident
// k_mailbox wavefront on a stream of its own: oc_mailbox_step posts a request (mailbox_post: the state and the actions as tagged
// 16-byte granules), waits for the tagged response lines and relaunches the kernel (mailbox_launch) when it has left for idleness or age.
// Part of liboc_amd.so: included by oc_amd.hip at file scope.  The kernel is mailbox.hpp.
#pragma once

// (at global scope: the opaque type of include/oc_amd.h)
struct OcMailbox {
    uint8_t* h;             // the mailbox (pinned host memory, mapped into the GPU's address space)
    uint8_t* d;             // its device address
    hipStream_t stream;     // the resident kernel's own stream
    const OcLayout* d_layout;
    int W, n_obj, horizon, device, max_pots;
    uint32_t seq;
    uint64_t idle_ticks, life_ticks;
};

namespace {
static_assert(OC_MB_STATE_IN == MB_IN && OC_MB_ACTIONS == MB_ACT && OC_MB_STATE_OUT == MB_OUT && OC_MB_REWARDS == MB_REW &&
              OC_MB_FLAGS == MB_FLAGS && OC_MB_EVENTS == MB_EV, "mailbox offsets of include/oc_amd.h");

// the request granules of `tag`: payload = n_state bytes of MB_IN + the two bytes of MB_ACT
void mailbox_post(OcMailbox* m, uint32_t tag, int n_state) {
    alignas(16) uint8_t pay[12 * MB_REQ_MAX + 4] = {0};
    memcpy(pay, m->h + MB_IN, (size_t)n_state);
    memcpy(pay + n_state, m->h + MB_ACT, 2);
    const int n_req = (n_state + 2 + 11) / 12;
    for (int g = 0; g < n_req; ++g) {
        alignas(16) uint32_t q[4];
        memcpy(q, pay + 12 * g, 12);
        q[3] = tag;
        typedef long long mb_i64x2 __attribute__((vector_size(16), aligned(16)));
        *reinterpret_cast<volatile mb_i64x2*>(m->h + MB_REQG + 16 * g) = *reinterpret_cast<const mb_i64x2*>(q);  // one movaps
    }
}

int mailbox_launch(OcMailbox* m) {
    *reinterpret_cast<volatile uint32_t*>(m->h + MB_ALIVE) = 1u;
    DISPATCH_NOBJ(m->n_obj, {
        constexpr int NO = NOBJ <= STEP1_MAX_PLANES ? NOBJ : 1;
        if (NOBJ <= STEP1_MAX_PLANES) {
            if (m->max_pots <= 2)
                hipLaunchKernelGGL((k_mailbox<NO, 2>), dim3(1), dim3(64), 0, m->stream, m->d_layout, m->d, m->W, m->horizon,
                                   m->idle_ticks, m->life_ticks);
            else
                hipLaunchKernelGGL((k_mailbox<NO, OC_MAX_POTS>), dim3(1), dim3(64), 0, m->stream, m->d_layout, m->d, m->W,
                                   m->horizon, m->idle_ticks, m->life_ticks);
        }
    });
    return check_launch("oc_mailbox: launch");
}
}  // namespace

extern "C" {

int oc_mailbox_open(const OcBatch* b, int horizon, OcMailbox** out) {
    int n_obj = 0;
    if (!out) return fail(OC_EINVAL, "oc_mailbox_open: NULL result pointer");
    *out = nullptr;
    if (int rc = check_batch(b, &n_obj)) return rc;
    if (b->n_layouts != 1 || n_obj > STEP1_MAX_PLANES) return fail(OC_EINVAL, "oc_mailbox_open: one layout, grids of at most 64 cells");
    if (int rc = check_horizon("oc_mailbox_open", horizon)) return rc;
    OcMailbox* m = new OcMailbox();
    if (hipGetDevice(&m->device) != hipSuccess || hipHostMalloc((void**)&m->h, MB_BYTES, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
        delete m;
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_mailbox_open: pinned host memory refused");
    }
    memset(m->h, 0, MB_BYTES);
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, m->device) != hipSuccess || khz <= 0) khz = 100000;  // 100 MHz
    if (hipHostGetDevicePointer((void**)&m->d, m->h, 0) != hipSuccess ||
        hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) {
        (void)hipHostFree(m->h);
        delete m;
        (void)hipGetLastError();
        return fail(OC_ELAUNCH, "oc_mailbox_open: device mapping / stream refused");
    }
    m->d_layout = b->d_layouts; m->W = b->width; m->n_obj = n_obj; m->horizon = horizon; m->seq = 0;
    m->max_pots = b->max_pots > 0 ? b->max_pots : OC_MAX_POTS;  // (hint of oc_batch_hints; unknown: the general instance)
    m->idle_ticks = (uint64_t)khz * 2;     // 2 ms without a request
    m->life_ticks = (uint64_t)khz * 2000;  // 2 s in any case
    if (int rc = mailbox_launch(m)) { (void)oc_mailbox_close(m); return rc; }
    *out = m;
    return OC_OK;
}

void* oc_mailbox_buffer(OcMailbox* m) { return m ? m->h : nullptr; }

int oc_mailbox_step(OcMailbox* m) {
    if (!m) return fail(OC_EINVAL, "oc_mailbox_step: NULL mailbox");
    uint32_t seq = m->seq + 1u;
    if (seq == MB_STOP || seq == 0u) seq = 1u;
    m->seq = seq;
    const int n_state = 16 * (1 + m->n_obj);
    const int n_words = (n_state + 28) / 4;  // payload dwords of the response
    // ---- the request: the caller's plain views (MB_IN, MB_ACT) as granules of {12 payload bytes, tag}, one aligned 16-byte
    //      store each (the kernel's lanes read one granule each with a single 16-byte load: payload and tag arrive together)
    mailbox_post(m, seq, n_state);
    // ---- the response: two 64-byte lines of {15 payload dwords, tag}
    volatile uint32_t* alive = reinterpret_cast<volatile uint32_t*>(m->h + MB_ALIVE);
    uint32_t spins = 0;
    struct timespec t0 = {0, 0};
    for (;;) {
        // the last dword of each response line carries the tag once the line has arrived (line 1 only when the payload needs it)
        int ok = __atomic_load_n(reinterpret_cast<uint32_t*>(m->h + MB_RSPG + 60), __ATOMIC_ACQUIRE) == seq;
        if (ok && n_words > 15) ok = __atomic_load_n(reinterpret_cast<uint32_t*>(m->h + MB_RSPG + 124), __ATOMIC_ACQUIRE) == seq;
        if (ok) break;
        __builtin_ia32_pause();
        if ((++spins & 0x3FFu) != 0u) continue;
        if (*alive == 0u) {  // the kernel has left (idle / lifetime): the next incarnation finds the request
            int dev = 0;
            (void)hipGetDevice(&dev);
            if (dev != m->device) (void)hipSetDevice(m->device);
            const int rc = mailbox_launch(m);
            if (dev != m->device) (void)hipSetDevice(dev);
            if (rc) return rc;
        }
        struct timespec now;
        clock_gettime(CLOCK_MONOTONIC, &now);
        if (t0.tv_sec == 0 && t0.tv_nsec == 0) t0 = now;
        else if ((now.tv_sec - t0.tv_sec) > 5) return fail(OC_ELAUNCH, "oc_mailbox_step: no answer from the resident kernel within 5 s");
    }
    uint8_t rsp[120];
    memcpy(rsp, m->h + MB_RSPG, 60);
    memcpy(rsp + 60, m->h + MB_RSPG + 64, 60);
    memcpy(m->h + MB_OUT, rsp, (size_t)n_state);
    memcpy(m->h + MB_REW, rsp + n_state, 16);
    memcpy(m->h + MB_FLAGS, rsp + n_state + 16, 4);
    memcpy(m->h + MB_EV, rsp + n_state + 20, 8);
    return OC_OK;
}

int oc_mailbox_close(OcMailbox* m) {
    if (!m) return OC_OK;
    mailbox_post(m, MB_STOP, 16 * (1 + m->n_obj));
    (void)hipStreamSynchronize(m->stream);
    (void)hipStreamDestroy(m->stream);
    (void)hipHostFree(m->h);
    (void)hipGetLastError();
    delete m;
    return OC_OK;
}

#ifdef OC_AMD_TUNING
// tuning builds: n back-to-back oc_mailbox_step calls from C (no Python / ctypes between them) -> microseconds per call
double oc_mailbox_bench(OcMailbox* m, int n) {
    struct timespec a, b;
    clock_gettime(CLOCK_MONOTONIC, &a);
    for (int i = 0; i < n; ++i)
        if (oc_mailbox_step(m)) return -1.0;
    clock_gettime(CLOCK_MONOTONIC, &b);
    return ((b.tv_sec - a.tv_sec) * 1e9 + (b.tv_nsec - a.tv_nsec)) / n * 1e-3;
}
#endif

}  // extern "C"
