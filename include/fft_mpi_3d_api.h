// fft_mpi_3d_api.h -- the reference's distributed-FFT API names (C++ linkage, as in
// /root/reference/3dmpifft_opt/include/fft_mpi_3d_api.h:68-86) as thin inline wrappers over the C-ABI of
// libdfft_mi355x.so (include/dfft.h).  The reference driver fftSpeed3d_c2c.cpp compiles unchanged against this header:
// same function names, argument meaning, plan member it pokes (plan->bufferDev1, fftSpeed3d_c2c.cpp:78), collective
// calling discipline (one host thread per local GPU) and error behaviour (print + exit, fft_mpi_common.h:31-103).
//
// Header-only on purpose: MPI_Comm is whatever <mpi.h> the application was built with (a real MPI, or
// include/dfft_mpi_shim/mpi.h), so no MPI type crosses the shared library's ABI.
#ifndef __FFT_MPI_3D_API_H__
#define __FFT_MPI_3D_API_H__

#include <cstring>
#include <mutex>
#include <vector>

#include "fft_mpi_common.h"

typedef struct fft_mpi_3d_plan {
    // members of the reference struct (fft_mpi_3d_api.h:11-66) that describe the plan; the rocFFT/hipFFT/templateFFT
    // handles have no counterpart here.
    int         N[3];
    int         locGPUIdx, devCountInNode, totalDevCount, globalDevIdx;
    int         mpiRank, mpiSize;
    bool        isLastDevice, isInplace;
    longInt64   maxDataCountInDevice;
    Complex *   inDev, *outDev, *bufferDev1, *bufferDev2, **nodeDataDev;
    TransInfo   tInfo;
    longInt64   lastExchangeN0, lastExchangeN1, lastExchangeN2;
    hipStream_t stream1;
    int         direction;
    dfft_plan_t handle;  // the MI355X-native plan
} * fft_mpi_3d_plan_p;

namespace dfft_api_detail {
// Process-wide state established by fft_mpi_init and consumed by plan creation (the reference keeps the equivalent
// in the caller's node_data[] array plus OpenMP's implicit team, fft_mpi_3d_api.cpp:80,190).
struct State {
    std::mutex               m;
    int                      total = 1, in_rank = 1, mpi_rank = 0, mpi_size = 1;
    bool                     have_id = false;
    bool                     use_ipc = false;          // DFFT_EXCHANGE=ipc | ipc-async: hipIpc communicator instead of RCCL
    bool                     ipc_async = false;
    char                     rccl_id[128];
    dfft_comm_t              local = nullptr;          // single-process: shared by all device threads
    std::vector<dfft_comm_t> rccl;                     // multi-process: one communicator rank per local device
};
inline State& state() {
    static State s;
    return s;
}
inline int first_dev_of_rank(int total, int mpi_size, int mpi_rank) {
    return mpi_rank * (int)ceil((double)total / mpi_size);  // fft_mpi_3d_api.cpp:57
}
}  // namespace dfft_api_detail

// getMaxDataCount (fft_mpi_3d_api.cpp:289-316)
inline longInt64 getMaxDataCount(int n0, int n1, int n2, int totalDevCount, bool isLastDevice) {
    return dfft_max_count(n0, n1, n2, totalDevCount, isLastDevice ? 1 : 0);
}

// getProperDeviceNum (fft_mpi_3d_api.h:77, fft_mpi_3d_api.cpp:232-272): shrink the device count until every device owns at least one
// X-plane of a ceil split (N0 % P != 0), hand the devices out to the ranks, print the reference's lines.
// Environment: DFFT_VIRTUAL_DEVICES=1 lets GPU_COUNT exceed the visible device count (devices are then shared
// round-robin exactly as the reference driver's hipSetDevice(globalIdx % devCount), fftSpeed3d_c2c.cpp:53).
inline void getProperDeviceNum(const longInt64* N, int iniDeviceNumInNode, int mpi_size, int mpi_rank, int& newDeviceCount,
                               int& newDeviceCountInNode) {
    int         real = dfft_device_count();
    const char* virt = getenv("DFFT_VIRTUAL_DEVICES");
    const bool  allow_virtual = virt && atoi(virt) != 0;
    if (iniDeviceNumInNode > real && !allow_virtual) {
        printf("The number of GPUs in rank %d is less than %d, so it will be set to %d (equal to your real device count).\n",
               mpi_rank, iniDeviceNumInNode, real);  // fft_mpi_3d_api.cpp:237
    }
    // (a distribution that leaves this rank without a device is the reference's "could not support this distribution of data,
    // exit!!", :265-268: DFFT_CHECK prints the library's message for it and exits the same way)
    DFFT_CHECK(dfft_proper_device_count(N, iniDeviceNumInNode, mpi_size, mpi_rank, allow_virtual ? -1 : real,
                                        &newDeviceCount, &newDeviceCountInNode));
    printf("allocate %d devices to node %d\n", newDeviceCountInNode, mpi_rank);  // :270
}

// getDataCountForNode (fft_mpi_3d_api.h:78, fft_mpi_3d_api.cpp:274-287): elements of the input slab of every device of this rank
// (ceil(N0 / P) X-planes each, the last device of the last rank takes the remainder), printed as the reference prints them.
inline void getDataCountForNode(longInt64 dataCountInNode[], const longInt64 N[], int mpiRank, int mpiSize, int deviceCount,
                                int deviceCountInNode) {
    for (int i = 0; i < deviceCountInNode; ++i) {
        // the reference marks the last device as "last rank, last local index" (:279); the C-ABI names it by its global index
        const bool last = mpiRank == mpiSize - 1 && i == deviceCountInNode - 1;
        dataCountInNode[i] = dfft_local_count(N, deviceCount, last ? deviceCount - 1 : 0);
        printf("data count in device %d of node %d: %lld\n", i, mpiRank, dataCountInNode[i]);  // :285
    }
}

// fft_mpi_init (fft_mpi_3d_api.cpp:3-39): device-count fix-up, per-device element counts, exchange set-up.
inline void fft_mpi_init(const longInt64* N, int iniDeviceNumInNode, MPI_Comm comm, int& newDeviceCount,
                         int& newDeviceCountInNode, longInt64 dataCountInNode[]) {
    using namespace dfft_api_detail;
    int mpi_size, mpi_rank;
    MPI_CHECK(MPI_Comm_size(comm, &mpi_size));
    MPI_CHECK(MPI_Comm_rank(comm, &mpi_rank));
    getProperDeviceNum(N, iniDeviceNumInNode, mpi_size, mpi_rank, newDeviceCount, newDeviceCountInNode);      // :21
    getDataCountForNode(dataCountInNode, N, mpi_rank, mpi_size, newDeviceCount, newDeviceCountInNode);        // :24
    State& s = state();
    std::lock_guard<std::mutex> lk(s.m);
    s.total = newDeviceCount;
    s.in_rank = newDeviceCountInNode;
    s.mpi_rank = mpi_rank;
    s.mpi_size = mpi_size;
    if (s.local) {
        dfft_comm_destroy(s.local);
        s.local = nullptr;
    }
    s.rccl.assign(newDeviceCountInNode, nullptr);
    s.have_id = false;
    if (newDeviceCount > 1) {
        if (mpi_size == 1) {
            DFFT_CHECK(dfft_comm_create_local(newDeviceCount, &s.local));
        } else {
            const char* ex = getenv("DFFT_EXCHANGE");
            s.use_ipc = ex && (strcmp(ex, "ipc") == 0 || strcmp(ex, "ipc-async") == 0);
            s.ipc_async = ex && strcmp(ex, "ipc-async") == 0;
            if (!s.use_ipc) {
                // the reference's dead ENABLE_RCCL branch (fft_mpi_3d_api.cpp:29-37) made live
                if (mpi_rank == 0) DFFT_CHECK(dfft_rccl_unique_id(s.rccl_id));
                MPI_CHECK(MPI_Bcast(s.rccl_id, 128, MPI_BYTE, 0, comm));
            }
            s.have_id = true;
        }
    }
}

// fft_mpi_alloc_local_memory (fft_mpi_3d_api.cpp:216-230)
inline Complex* fft_mpi_alloc_local_memory(int count, int flag) {
    if (flag != ALLOC_CPU && flag != ALLOC_DEV) {
        printf("Fail to allocate memory!\n");
        exit(EXIT_FAILURE);
    }
    void* p = dfft_alloc(count, DFFT_F64, flag);
    if (!p) {
        fprintf(stderr, "[%s:%d] allocation of %d elements failed: %s\n", __FILE__, __LINE__, count, dfft_last_error());
        exit(EXIT_FAILURE);
    }
    return (Complex*)p;
}

// fft_mpi_plan_dft_c2c_3d (fft_mpi_3d_api.cpp:41-141).  The calling thread's current HIP device owns the plan.
inline fft_mpi_3d_plan_p fft_mpi_plan_dft_c2c_3d(longInt64 n0, longInt64 n1, longInt64 n2, Complex* in, Complex* out,
                                                 Complex** node_data, MPI_Comm comm, int devIdx, int devCountInNode,
                                                 int totalDevCount, int direction) {
    using namespace dfft_api_detail;
    fft_mpi_3d_plan_p plan = new fft_mpi_3d_plan;
    plan->N[0] = (int)n0;
    plan->N[1] = (int)n1;
    plan->N[2] = (int)n2;
    plan->direction = direction;
    plan->locGPUIdx = devIdx;
    plan->devCountInNode = devCountInNode;
    plan->totalDevCount = totalDevCount;
    MPI_CHECK(MPI_Comm_rank(comm, &plan->mpiRank));
    MPI_CHECK(MPI_Comm_size(comm, &plan->mpiSize));
    plan->globalDevIdx = first_dev_of_rank(totalDevCount, plan->mpiSize, plan->mpiRank) + devIdx;
    plan->isLastDevice = (plan->globalDevIdx == totalDevCount - 1);
    plan->maxDataCountInDevice = getMaxDataCount((int)n0, (int)n1, (int)n2, totalDevCount, plan->isLastDevice);
    plan->inDev = in;
    plan->outDev = out;
    plan->isInplace = (out == NULL || out == in);
    plan->lastExchangeN2 = n2;
    plan->lastExchangeN0 = n0 - (totalDevCount - 1) * (longInt64)ceil((double)n0 / totalDevCount);
    plan->lastExchangeN1 = n1 - (totalDevCount - 1) * (longInt64)ceil((double)n1 / totalDevCount);

    dfft_comm_t c = nullptr;
    if (totalDevCount > 1) {
        State& s = state();
        bool   create = false;
        char   id[128];
        {
            std::lock_guard<std::mutex> lk(s.m);
            if (s.local) {
                c = s.local;
            } else {
                if (!s.have_id || devIdx >= (int)s.rccl.size()) {
                    fprintf(stderr, "[%s:%d] fft_mpi_init must run before plan creation\n", __FILE__, __LINE__);
                    exit(EXIT_FAILURE);
                }
                c = s.rccl[devIdx];
                if (!c) {
                    create = true;
                    memcpy(id, s.rccl_id, sizeof(id));
                }
            }
        }
        if (create) {
            // collective over every device of every rank: must not be called under the lock (the other device
            // threads of this process have to get in here too); slot devIdx belongs to this device thread alone
            if (s.use_ipc) DFFT_CHECK(dfft_comm_create_ipc(totalDevCount, plan->globalDevIdx, s.ipc_async ? 1 : 0, &c));
            else DFFT_CHECK(dfft_comm_create_rccl(id, totalDevCount, plan->globalDevIdx, &c));
            std::lock_guard<std::mutex> lk(s.m);
            s.rccl[devIdx] = c;
        }
    }
    // DFFT_OVERLAP=1: forward plans pipeline the exchange behind t0 and t3 behind the tail of the exchange (the printed
    // t2 is then the exposed remainder).  Default: the reference's serial t0 -> t1 -> t2 -> t3 stage structure.
    // DFFT_ANY_LENGTH=1: also accept axis lengths that are not 7-smooth (Bluestein, DFFT_PLAN_ANY_LENGTH).  Default off.
    const char*    ov = getenv("DFFT_OVERLAP");
    const char*    al = getenv("DFFT_ANY_LENGTH");
    const unsigned plan_flags = ((ov && *ov && *ov != '0' && totalDevCount > 1) ? DFFT_PLAN_OVERLAP : DFFT_PLAN_DEFAULT) |
                                ((al && *al && *al != '0') ? DFFT_PLAN_ANY_LENGTH : 0u);
    DFFT_CHECK(dfft_plan_create(&plan->handle, n0, n1, n2, DFFT_F64, direction, in, out, c, plan->globalDevIdx,
                                totalDevCount, plan_flags));
    // plan-time placement of the internal hand-over buffer (dfft_plan_tune, a few X-pass kernel launches): done here so that
    // `sh speedTest.sh 1 X Y Z` times the same configuration as bench.py.  The probe launches of a forward plan write into `out`;
    // dfft_plan_tune sets its contents aside and puts them back (like the reference's, this plan creation leaves `out` as it found
    // it), borrows at most a quarter of the free device memory (DFFT_TUNE_MEM_PCT) and 32 candidates (DFFT_TUNE_TRIES), and is
    // skipped for in-place plans.  DFFT_TUNE=0 switches it off.
    if (!plan->isInplace) DFFT_CHECK(dfft_plan_tune(plan->handle));
    plan->bufferDev1 = (Complex*)dfft_plan_buffer1(plan->handle);
    plan->bufferDev2 = (Complex*)dfft_plan_result(plan->handle);
    plan->stream1 = (hipStream_t)dfft_plan_stream(plan->handle);
    plan->nodeDataDev = node_data;
    if (node_data) node_data[devIdx] = plan->bufferDev1;  // fft_mpi_3d_api.cpp:80
    plan->tInfo.rcount = new longInt64[totalDevCount];
    plan->tInfo.roffset = new longInt64[totalDevCount];
    plan->tInfo.scount = new longInt64[totalDevCount];
    plan->tInfo.soffset = new longInt64[totalDevCount];
    DFFT_CHECK(dfft_exchange_layout(n0, n1, n2, totalDevCount, plan->globalDevIdx, direction, plan->tInfo.scount,
                                    plan->tInfo.soffset, plan->tInfo.rcount, plan->tInfo.roffset));
    return plan;
}

// fft_mpi_execute_dft_3d_c2c (fft_mpi_3d_api.cpp:181-214): blocking, stage-timed, prints the "t0: ..." line on forward.
inline void fft_mpi_execute_dft_3d_c2c(fft_mpi_3d_plan_p p) {
    DFFT_CHECK(dfft_execute(p->handle, DFFT_EXEC_SYNC_STAGES | DFFT_EXEC_PRINT));
}

// fft_mpi_destroy_plan (fft_mpi_3d_api.cpp:143-179)
inline void fft_mpi_destroy_plan(fft_mpi_3d_plan_p plan) {
    delete[] plan->tInfo.rcount;
    delete[] plan->tInfo.scount;
    delete[] plan->tInfo.roffset;
    delete[] plan->tInfo.soffset;
    DFFT_CHECK(dfft_plan_destroy(plan->handle));
    delete plan;
}

// Declared by the reference but never defined there (fft_mpi_3d_api.h:69,73); provided here.
inline void fft_mpi_cleanup(void) {
    using namespace dfft_api_detail;
    State& s = state();
    std::lock_guard<std::mutex> lk(s.m);
    if (s.local) dfft_comm_destroy(s.local);
    s.local = nullptr;
    for (auto& c : s.rccl) {
        if (c) dfft_comm_destroy(c);
        c = nullptr;
    }
}
inline longInt64 fft_mpi_local_size_3d(longInt64 n0, longInt64 n1, longInt64 n2, MPI_Comm comm, longInt64* local_n0,
                                       longInt64* local_0_start) {
    using namespace dfft_api_detail;
    int rank, size;
    MPI_CHECK(MPI_Comm_rank(comm, &rank));
    MPI_CHECK(MPI_Comm_size(comm, &size));
    State& s = state();
    const int total = s.total > 0 ? s.total : size;
    const int g = first_dev_of_rank(total, size, rank);
    DFFT_CHECK(dfft_local_size(n0, n1, n2, total, g, local_n0, local_0_start, nullptr, nullptr));
    return dfft_max_count(n0, n1, n2, total, g == total - 1);
}

#endif  // __FFT_MPI_3D_API_H__
