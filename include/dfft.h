/* dfft.h -- C-ABI of libdfft_mi355x.so: the MI355X-native slab 3D C2C FFT.
 *
 * This is the drop-in boundary for the hot path of lueelu/DistributedFFT's 3dmpifft_opt
 * (t0 batched 2D YZ FFT -> t1 pack -> t2 all-to-all -> t3 batched 1D X FFT).  Every entry point names the reference
 * interface it replaces (paths relative to /root/reference/3dmpifft_opt/include/).  The reference API has C++ linkage
 * (fft_mpi_3d_api.h:68-79); thin C++ wrappers with the original names live in include/fft_mpi_3d_api.h and call
 * straight into these functions, so the reference driver (fftSpeed3d_c2c.cpp) recompiles unchanged against this
 * library.  Plain pointers and sizes only: no torch, no MPI, no C++ types in any signature.
 *
 * Error handling: functions returning int return 0 on success and a negative DFFT_E* code on failure (the C++
 * wrappers reproduce the reference behaviour: print "[file:line] ... failed" and exit(EXIT_FAILURE),
 * fft_mpi_common.h:31-103).  dfft_last_error() returns a thread-local message for the last failure.
 *
 * Layout contract, device g of P, xl = ceil(N0/P), yl = ceil(N1/P), last device takes the rest:
 *   forward  input  : [x_local][N1][N2]  (x slowest)            element (xi*N1 + y)*N2 + z
 *   forward  output : [y_local][N2][N0]  (kx fastest)           element (yy*N2 + z)*N0 + kx   (transposed, Y-slabbed)
 *   backward input  : the forward output layout;  backward output: the forward input layout.  Both unnormalised.
 */
#ifndef DFFT_H
#define DFFT_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFFT_FORWARD 1   /* fft_mpi_common.h:18  FORWARD  */
#define DFFT_BACKWARD (-1) /* fft_mpi_common.h:19  BACKWARD */
#define DFFT_ALLOC_HOST 1  /* fft_mpi_common.h:15  ALLOC_CPU */
#define DFFT_ALLOC_DEV (-1) /* fft_mpi_common.h:16  ALLOC_DEV */

#define DFFT_F64 0 /* Complex = double[2] (fft_mpi_common.h:21); the only precision the reference has */
#define DFFT_F32 1 /* float[2]; BASELINE config 5 */

/* error codes */
#define DFFT_OK 0
#define DFFT_EINVAL (-1)      /* bad argument / unsupported size */
#define DFFT_EHIP (-2)        /* a HIP runtime call failed */
#define DFFT_ERCCL (-3)       /* an RCCL call failed */
#define DFFT_ENOGPU (-4)      /* no usable gfx950 device: the product path has no CPU fallback */
#define DFFT_ECOMM (-5)       /* bootstrap / rendezvous failure */
#define DFFT_EUNSUPPORTED (-6)

/* plan flags */
#define DFFT_PLAN_DEFAULT 0u
#define DFFT_PLAN_UNFUSED 1u        /* reference stage structure: Y-FFT in place, separate pack (t1), separate tile transpose
                                       in t3.  Default is fused (pack and transpose folded into the FFT kernels' stores). */
#define DFFT_PLAN_INPUT_FROM_IN 2u  /* every execute re-reads the caller's `in` (first pass runs out-of-place in -> bufferDev1)
                                       instead of consuming bufferDev1; out-of-place plans only.  Same HBM traffic. */
#define DFFT_PLAN_OVERLAP 4u        /* P > 1: the exchange runs in pieces on a second stream -- X-plane parts overlapped with
                                       the YZ stage, Y sub-blocks with the X stage (forward plans; backward plans that also
                                       set DFFT_PLAN_INPUT_FROM_IN).  Results are bit-identical to the serial pipeline. */
#define DFFT_PLAN_NATURAL 8u        /* input AND output in the natural X-slab layout [x_local][N1][N2] (both directions):
                                       the un-transposed output the reference declares (fft_mpi_local_size_3d,
                                       fft_mpi_3d_api.h:73) but never implements.  Costs a second all-to-all when P > 1. */
#define DFFT_PLAN_ANY_LENGTH 16u    /* also accept axes of dfft_length_kind 3 (Bluestein, see dfft_fft1d_any).  A plan with such an
                                       axis runs the un-fused stage structure like a four-step plan: UNFUSED is forced, OVERLAP
                                       dropped, NATURAL rejected (DFFT_EUNSUPPORTED).  Without a kind-3 axis the flag changes nothing
                                       (bit-identical results).  Not accepted by dfft_plan_create_r2c. */

/* execute flags */
#define DFFT_EXEC_ASYNC 0u          /* enqueue on the plan's stream and return */
#define DFFT_EXEC_SYNC_STAGES 1u    /* hipDeviceSynchronize-style host timing per stage, like fft_mpi_3d_api.cpp:184-201 */
#define DFFT_EXEC_PRINT 2u          /* print the reference's "t0: .. t1: .. t2: .. t3: .. total: .." line (forward only) */
#define DFFT_EXEC_NO_TIMING 4u      /* do not record the stage-boundary events (dfft_stage_times is then unavailable): a
                                       production loop of small transforms is launch-bound, and the 5-6 event records per
                                       execute are as many queue packets as the kernels themselves */

typedef struct dfft_plan_s* dfft_plan_t;
typedef struct dfft_comm_s* dfft_comm_t;

/* ---- library / device ------------------------------------------------------------------------------------------ */
const char* dfft_version(void);
const char* dfft_last_error(void);
/* Number of visible HIP devices (0 if none).  hipGetDeviceCount in fftSpeed3d_c2c.cpp:33-34. */
int dfft_device_count(void);
/* PCI address ("domain:bus:device.function", hipDeviceGetPCIBusId) of HIP device `device` (-1: the calling thread's current
 * device): the identity a multi-process launch compares to prove that its ranks sit on distinct GPUs -- ordinals do not
 * (HIP_VISIBLE_DEVICES renumbers them per process).  Returns 0 and a NUL-terminated string in buf[0..len). */
int dfft_device_pci_bus_id(int device, char* buf, int len);
/* 1 if FFT length n is supported: any product of 2, 3, 5, 7 up to 4096 (tuned plans for the lengths listed in
 * csrc/dfft_plans.h, a run-time-scheduled kernel for the rest) -- the single-pass range of the reference's generator --
 * and, above 4096, every product of two tuned lengths up to 2^24 (two-pass "four-step" plans, csrc/dfft_long.hip; the
 * reference's multi-upload plans, templateFFT.cpp:3972-4106).  3D plans with such an axis run the un-fused stage structure. */
int dfft_length_supported(long long n);
/* How length n is computed: 1 single-pass (7-smooth, n <= 4096: where dfft_length_supported is 1 up to 4096), 2 four-step (the rest of
 * dfft_length_supported), 3 Bluestein (every other n from 1 to 2^23, n = 1 included: a scaled copy; dfft_fft1d_any and plans with
 * DFFT_PLAN_ANY_LENGTH), 0 none.  Pure host arithmetic. */
int dfft_length_kind(long long n);
/* The padded length M >= 2n - 1 a Bluestein transform of length n runs on (1 for n = 1; the smallest tuned single-pass length for
 * n <= 2048, the smallest four-step length above), or 0 if n is not of kind 3.  Pure host arithmetic. */
long long dfft_bluestein_length(long long n);
/* How a real transform of length n is computed (dfft_rfft1d, dfft_plan_create_r2c_any): 1 half-length (n even, n/2 a single-pass length:
 * the row kernels of dfft_plan_create_r2c); 2 paired single-pass (the odd 7-smooth n <= 4096, and n = 2: two real rows a, b packed into
 * one complex row a + i b share one n-point transform); 3 paired multi-pass (the n-point four-step or Bluestein transform, n = 1
 * included); 0 none.  Pure host arithmetic. */
int dfft_real_form(long long n);

/* ---- slab bookkeeping: pure host arithmetic, callable without a GPU ------------------------------------------------ */
/* getProperDeviceNum (fft_mpi_3d_api.cpp:232-272): shrink the device count when N0 % P != 0 so every device but the
 * last owns ceil(N0/P) planes.  real_devices < 0 skips the clamp to the visible device count. */
int dfft_proper_device_count(const long long N[3], int ini_devices_in_rank, int nranks, int rank, int real_devices,
                             int* new_total, int* new_in_rank);
/* getDataCountForNode (fft_mpi_3d_api.cpp:274-287): elements held by global device idx before the transform. */
long long dfft_local_count(const long long N[3], int total_devices, int global_idx);
/* getMaxDataCount (fft_mpi_3d_api.cpp:289-316): elements each of in/out/bufferDev1 must hold. */
long long dfft_max_count(long long n0, long long n1, long long n2, int total_devices, int is_last_device);
/* Per-peer exchange counts/offsets in elements (tInfo, fft_mpi_3d_api.cpp:84-133; receive offsets :618-625).
 * Arrays have total_devices entries.  direction = DFFT_FORWARD or DFFT_BACKWARD. */
int dfft_exchange_layout(long long n0, long long n1, long long n2, int total_devices, int global_idx, int direction,
                         long long* scount, long long* soffset, long long* rcount, long long* roffset);
/* The messages of ONE piece of the overlapped exchange (DFFT_PLAN_OVERLAP) as device global_idx issues them: X-plane part
 * `part` when every device cuts its X slab into parts of `part_planes` planes, restricted to Y sub-block `ycut` of `ycuts`
 * (or all sub-blocks for ycut = -1).  Message m goes to / comes from peer[m]; offsets/counts in elements.
 *   forward : send buffer packed [k][dst][x][y in k][N2] ([dst][x][y][N2] for ycuts = 1), receive buffer [k][x][y in k][N2]
 *   backward: the mirror image -- send buffer [k][x][y in k][N2], receive buffer [k][src][x][y in k][N2]
 * Both ends enumerate the messages of a pair in the same order.  Returns the number of messages, or a negative error.
 * (Refines slabAlltoall's per-peer chunks, fft_mpi_3d_api.cpp:610-672, into the pieces the pipeline overlaps.) */
int dfft_exchange_part_layout(long long n0, long long n1, long long n2, int total_devices, int global_idx, int direction,
                              long long part_planes, int part, int ycuts, int ycut, int max_msgs, int* peer,
                              long long* soffset, long long* scount, long long* roffset, long long* rcount);
/* local extents: x planes owned before / y rows owned after the forward transform, and their global starts.
 * (the declared-but-never-defined fft_mpi_local_size_3d, fft_mpi_3d_api.h:73) */
int dfft_local_size(long long n0, long long n1, long long n2, int total_devices, int global_idx, long long* local_n0,
                    long long* local_0_start, long long* local_n1, long long* local_1_start);

/* ---- exchange communicators (t2) -------------------------------------------------------------------------------------
 * LOCAL : all P devices are driven by threads of this process (reference: OpenMP thread per GPU + hipMemcpyPeerAsync,
 *         fft_mpi_3d_api.cpp:613-630).  Also serves P "virtual" devices sharing one physical GPU (parity tests).
 * RCCL  : one communicator rank per device, any process layout; replaces the MPI_Isend/Irecv on device pointers
 *         (fft_mpi_3d_api.cpp:635-672) with grouped ncclSend/ncclRecv over xGMI. */
int dfft_comm_create_local(int total_devices, dfft_comm_t* comm);
/* 128-byte RCCL unique id; rank 0 creates it and the host distributes it (torch.distributed, MPI, dfft_boot_*). */
int dfft_rccl_unique_id(char id[128]);
int dfft_comm_create_rccl(const char id[128], int total_devices, int global_idx, dfft_comm_t* comm);
/* IPC   : one process per device WITHOUT RCCL: the receive buffers are shared through hipIpc handles (exchanged over the
 *         dfft_boot_* rendezvous, which must describe exactly these processes), peers push their chunks with device-to-device
 *         copies (SDMA engines, no CUs), and the processes synchronise through the rendezvous' barrier -- the cross-process
 *         twin of the LOCAL communicator, i.e. the reference's MPI path with hipMemcpy instead of UCX (fft_mpi_3d_api.cpp:
 *         635-672).  Host-synchronising, so slower than RCCL for small messages; it also works with several processes sharing
 *         one GPU, which is how the multi-process path is tested on a single-GPU machine.  Plan creation and destruction are
 *         collective over the processes.  async_exchange != 0: the barriers become flag words in IPC-shared fine-grained
 *         memory, published and awaited by one-wave kernels on the plan's stream, so the exchange is stream-ordered like
 *         RCCL's (nothing blocks the host, DFFT_PLAN_OVERLAP overlaps) while the data still moves by copy engines. */
int dfft_comm_create_ipc(int total_devices, int global_idx, int async_exchange, dfft_comm_t* comm);
/* What a communicator actually is, as the transport reports it (launch diagnostics: a multi-GPU benchmark must be able to
 * prove which back-end ran and over how many ranks).  kind: 0 LOCAL, 1 RCCL, 2 IPC (host-synchronised), 3 IPC (stream-ordered);
 * size/rank: for RCCL the values of ncclCommCount / ncclCommUserRank (not the arguments the caller passed), otherwise the
 * creation arguments; device: HIP device ordinal the communicator is bound to (ncclCommCuDevice for RCCL, -1 for LOCAL).
 * Any output pointer may be NULL.  (The reference has no counterpart: MPI_Comm_size/rank, fftSpeed3d_c2c.cpp:20-21.) */
int dfft_comm_info(dfft_comm_t comm, int* kind, int* size, int* rank, int* device);
int dfft_comm_destroy(dfft_comm_t comm);

/* ---- memory ------------------------------------------------------------------------------------------------------------
 * fft_mpi_alloc_local_memory (fft_mpi_3d_api.cpp:216-230); count in complex elements of dtype. */
void* dfft_alloc(long long count, int dtype, int flag);
int dfft_free(void* p, int flag);

/* ---- plan / execute ------------------------------------------------------------------------------------------------------
 * fft_mpi_plan_dft_c2c_3d (fft_mpi_3d_api.cpp:41-141).  `in`/`out` are device buffers of dfft_max_count elements owned
 * by the caller; out == NULL or out == in selects in-place (bufferDev2 = in).  The plan allocates bufferDev1 and copies
 * `in` into it (input is captured at plan time or by writing dfft_plan_buffer1()).  comm may be NULL when
 * total_devices == 1.  The calling thread's current HIP device is the plan's device.
 * Buffer contract: any element-aligned pointers (fp32 buffers that are only 8-byte aligned run the scalar column kernels instead of the
 * column-pair ones: same results to rounding, lower bandwidth); in place (out == in or NULL) or out of place; byte ranges that overlap
 * only partly: DFFT_EINVAL, checked over dfft_max_count elements before the device is queried; with out != in and
 * DFFT_PLAN_INPUT_FROM_IN, `in` is never written; nothing outside the dfft_max_count elements of `in` and `out` is written. */
int dfft_plan_create(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in,
                     void* out, dfft_comm_t comm, int global_idx, int total_devices, unsigned flags);
/* Real-to-complex (direction DFFT_FORWARD) / complex-to-real (DFFT_BACKWARD) slab plan: the C2C contract above with the last axis
 * halved on the complex side, Nh = N2/2 + 1 (no counterpart in the reference, which is C2C only; heFFTe's fft3d_r2c).
 *   R2C input : real    [x_local][N1][N2]   element (xi*N1 + y)*N2 + z
 *   R2C output: complex [y_local][Nh][N0]   element (yy*Nh + kz)*N0 + kx  = numpy.fft.rfftn(x)[kx, y0 + yy, kz]
 *   C2R       : the R2C output layout -> the R2C input layout, unnormalised: N0*N1*N2 * numpy.fft.irfftn(X, s=(N0, N1, N2)) for ANY input
 *               (inverse C2C along X, then Y, then C2R along Z; the imaginary parts of the kz = 0 and kz = N2/2 bins are ignored).
 * DFFT_F64: double reals / double[2] bins; DFFT_F32: float / float[2].  `in` and `out` hold at least the counts of dfft_r2c_counts
 * (real side / complex side); the plan touches nothing beyond them.  Out of place only (out == NULL or out == in: DFFT_EINVAL).
 * Supported: N2 even with N2/2 a length dfft_length_supported accepts, at most 4096 (so N2 <= 8192); N0, N1 single-pass lengths
 * (<= 4096); flags DFFT_PLAN_DEFAULT or DFFT_PLAN_INPUT_FROM_IN; everything else DFFT_EUNSUPPORTED.  Arguments are checked before
 * the device is queried.  Returns an ordinary plan: dfft_execute, dfft_plan_sync, dfft_plan_set_scale, dfft_stage_times,
 * dfft_plan_buffer1 (the captured real slab of an R2C plan, the captured bins of a C2R plan), dfft_plan_result, dfft_plan_describe
 * ("pipeline=r2c" / "pipeline=c2r") and dfft_plan_destroy work on it with the C2C semantics; dfft_plan_tune is a no-op (no hand-over
 * buffer to place) and dfft_kernel_times returns DFFT_EUNSUPPORTED. */
int dfft_plan_create_r2c(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in,
                         void* out, dfft_comm_t comm, int global_idx, int total_devices, unsigned flags);
/* dfft_plan_create_r2c with the real axis N2 of any dfft_real_form != 0 (N2 >= 2): same arguments, layouts (dfft_r2c_counts,
 * Nh = N2/2 + 1), flags (DFFT_PLAN_DEFAULT, DFFT_PLAN_INPUT_FROM_IN) and limits on N0 and N1 (single-pass).  For N2 of form 1 the plan is
 * exactly dfft_plan_create_r2c's.  Forms 2 and 3 run the Z stage on pairs of rows (rows pair up across plane boundaries), each pair
 * through one N2-point complex transform; the plan owns the Bluestein tables and the scratch of one cache chunk of rows, so
 * dfft_execute allocates nothing.  Each row's rounding error is bounded relative to its pair's combined magnitude.
 * dfft_plan_describe appends "real_form=<f>" and, for form 3, "complex_form=four-step/<a>x<b>" or "complex_form=bluestein/M<M>/<fused|
 * multi-pass>".  Arguments are checked before the device is queried. */
int dfft_plan_create_r2c_any(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, int direction, void* in,
                             void* out, dfft_comm_t comm, int global_idx, int total_devices, unsigned flags);
/* ---- spectral-filter (FFT convolution) plans ---------------------------------------------------------------------------------------
 * y = ifftn( fftn(x) * H ), numpy conventions (normalised: H == 1 gives y == x), C2C, DFFT_F64 / DFFT_F32, slab-decomposed like
 * dfft_plan_create.  in / out: device buffers in the X-slab layout [x_local][N1][N2] holding dfft_local_count elements; out == in or
 * NULL: in place.  `in` is read at every execute (no capture at plan time) and is left alone when out != in.
 * Pipeline: forward YZ stage -> (P > 1: exchange) -> X stage IN PLACE on the slab [x][y_local][N2] (forward X transform, multiply by the
 * plan's filter copy, inverse X transform: one kernel for N0 = 64, 128, 256, 384, 512, 768, 1024, three launches otherwise or with
 * DFFT_CONV_FUSED=0, read at plan creation) -> (exchange) -> inverse YZ stage.  Execute allocates nothing.
 * Accepted: every axis of dfft_length_kind 1; P >= 1 on any communicator; flags DFFT_PLAN_DEFAULT only.  Any other flag and axes of
 * kind 0, 2 or 3: DFFT_EUNSUPPORTED; NULL plan / in, sizes < 1, a bad dtype or device index: DFFT_EINVAL -- all checked before the
 * device is queried (then DFFT_ENOGPU without one).
 * The handle is an ordinary plan: dfft_execute (ASYNC / SYNC_STAGES / NO_TIMING; DFFT_EINVAL before a filter is set), dfft_plan_sync,
 * dfft_plan_stream, dfft_stage_times (t = forward YZ stage, both exchanges, X stage, inverse YZ stage), dfft_plan_describe
 * ("pipeline=conv xconv=fused|multi filter=complex|real|unset ...") and dfft_plan_destroy work on it.  dfft_plan_set_scale(s) multiplies
 * the output by s; the factor is folded into the filter copy, so it TAKES EFFECT AT THE NEXT dfft_conv_set_filter / dfft_conv_set_kernel
 * (the stored copy is not re-folded).  dfft_plan_tune is a no-op (the X stage works in place: no placement to choose);
 * dfft_kernel_times returns DFFT_EUNSUPPORTED, dfft_plan_buffer1 / dfft_plan_result / dfft_plan_workbuf NULL.
 * Buffer contract: any element-aligned pointers; in place (out == in or NULL) or out of place; byte ranges that overlap only partly:
 * DFFT_EINVAL (over dfft_local_count elements, before the device is queried); with out != in, `in` is never written; nothing outside
 * the dfft_local_count elements of `out` is written.  The one-kernel X stage moves fp32 elements in pairs: a P = 1 plan whose fp32 `out`
 * is only 8-byte aligned runs the three-launch stage instead (dfft_plan_describe: xconv=multi; dfft_conv_fused_applies). */
#define DFFT_FILTER_COMPLEX 0
#define DFFT_FILTER_REAL 1
int dfft_plan_create_conv(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, void* in, void* out,
                          dfft_comm_t comm, int global_idx, int total_devices, unsigned flags);
/* Diagnostics (host-only arithmetic): 1 if the one-kernel X stage serves a slab of `rows` rows per X plane, `ncols` columns, element
 * strides plane / pitch and row rotation `rot` at the addresses in / out, else 0 (the plan then runs the three-launch stage).  A fused
 * length N0; DFFT_F32 runs on column PAIRS with 16-byte accesses: even ncols, plane, pitch and rot, and in / out on 16-byte boundaries. */
int dfft_conv_fused_applies(int dtype, long long n0, long long rows, long long ncols, long long plane, long long pitch, int rot,
                            const void* in, const void* out);
/* Elements of this device's share of the filter: local_n1 * N2 * N0 (host-only arithmetic, no device needed); -1 for bad arguments. */
long long dfft_conv_filter_count(long long n0, long long n1, long long n2, int total_devices, int global_idx);
/* The filter's spectrum, given in the layout a forward dfft_plan_create plan of the same shape / communicator returns on this device:
 * element (yy*N2 + kz)*N0 + kx = H[kx, y0 + yy, kz].  kind DFFT_FILTER_COMPLEX: elements of the plan's complex type;
 * DFFT_FILTER_REAL: its real type (H real: Green's functions, Gaussians, masks -- half the filter bytes per execute).
 * The plan keeps a PRIVATE copy, re-laid-out for its X stage and with 1/(N0*N1*N2) and the plan's scale folded in; `h` may be freed or
 * changed afterwards.  May be called again between executes.  Synchronises the device; never called from dfft_execute. */
int dfft_conv_set_filter(dfft_plan_t plan, const void* h, int kind);
/* Convenience: the filter is fftn(k) of a real-space kernel k given in the plan's INPUT layout (complex type).  The plan runs its own
 * forward half on it (collective over the communicator like an execute) and keeps a complex filter copy.  Synchronises. */
int dfft_conv_set_kernel(dfft_plan_t plan, const void* k);

/* ---- real-field spectral-filter plans ----------------------------------------------------------------------------------------------
 * y = irfftn( rfftn(x) * H, s = (N0, N1, N2) ), numpy conventions (H == 1 gives y == x), for REAL fields: half the field's memory and half
 * the bytes of every pass and of both exchanges of dfft_plan_create_conv on the widened field, and no widening / narrowing pass.
 * in / out: device buffers of the plan's REAL type (double / float) in the X-slab layout [x_local][N1][N2], dfft_local_count reals;
 * out == in or NULL: in place.  `in` is read at every execute (nothing is captured at plan time) and left alone when out != in.
 * The result is numpy's for ANY complex H: the inverse runs C2C along X and Y, then C2R along Z, which ignores the imaginary parts of the
 * kz = 0 and kz = N2/2 bins (the backward order of dfft_plan_create_r2c).
 * Pipeline: R2C rows + Y columns per cache chunk -> (P > 1: pack, exchange) -> the X stage of dfft_plan_create_conv in place on the half
 * spectrum -> (exchange, unpack) -> inverse Y columns + C2R rows per cache chunk.  The half spectrum is private to the plan and
 * Nc >= Nh = N2/2 + 1 bins wide, its extra columns zero (Nc even, and a multiple of up to one 128-byte line where that pads at most
 * Nh/32 columns: Nh = 257 -> 264); dfft_plan_describe reports it as width=<Nc>.  Execute allocates nothing.
 * Accepted: N0, N1 of dfft_length_kind 1; N2 of dfft_real_form 1 (even, N2/2 a single-pass length); P >= 1 on any communicator; flags
 * DFFT_PLAN_DEFAULT only.  Every other flag, N0 / N1 of kind 0, 2 or 3 and N2 of real form 0, 2 or 3 (odd, N2 = 2, N2/2 beyond the
 * single-pass range: REFUSED, unlike dfft_plan_create_r2c_any): DFFT_EUNSUPPORTED; NULL plan / in, sizes < 1, a bad dtype or device
 * index: DFFT_EINVAL -- all checked before the device is queried (then DFFT_ENOGPU without one).
 * The handle is an ordinary plan with the semantics of dfft_plan_create_conv's: dfft_execute (ASYNC / SYNC_STAGES / NO_TIMING;
 * DFFT_EINVAL before a filter is set), dfft_plan_sync, dfft_plan_stream, dfft_stage_times (the same four stages), dfft_plan_set_scale
 * (takes effect at the next dfft_conv_set_filter / dfft_conv_set_kernel), dfft_plan_describe ("pipeline=conv-real xconv=fused|multi
 * filter=complex|real|unset width=<Nc> ...") and dfft_plan_destroy; dfft_plan_tune is a no-op, dfft_kernel_times returns
 * DFFT_EUNSUPPORTED, dfft_plan_buffer1 / dfft_plan_result / dfft_plan_workbuf NULL.
 * dfft_conv_set_filter(plan, h, kind) takes h in the layout a forward dfft_plan_create_r2c plan of the same shape / communicator returns
 * on this device: element (yy*Nh + kz)*N0 + kx = H[kx, y0 + yy, kz], dfft_conv_real_filter_count elements -- of the plan's complex type,
 * or of its real type with DFFT_FILTER_REAL.  The private copy has 1/(N0*N1*N2) and the plan's scale folded in.
 * dfft_conv_set_kernel(plan, k) takes a REAL kernel k in the plan's input layout (the real type) and keeps rfftn(k) as a complex filter;
 * collective like an execute. */
int dfft_plan_create_conv_real(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, void* in, void* out,
                               dfft_comm_t comm, int global_idx, int total_devices, unsigned flags);
/* Elements of this device's share of a real-field plan's filter: local_n1 * (N2/2 + 1) * N0 (host-only arithmetic); -1 for bad arguments. */
long long dfft_conv_real_filter_count(long long n0, long long n1, long long n2, int total_devices, int global_idx);

/* ---- multi-output real-field spectral-filter plans ---------------------------------------------------------------------------------
 * K real outputs of ONE real input through ONE base filter and per-output separable factors:
 *     y_k = irfftn( rfftn(x) * H * (a_k (x) b_k (x) c_k), s = (N0, N1, N2) ),   k = 0 .. noutputs-1,
 * a_k, b_k, c_k complex vectors along kx, ky, kz (i*k for a gradient component, a separable window, or ones) -- a potential and its
 * three force components, say.  The input is transformed once, the filter copy is kept once, the forward exchange runs once; only the
 * inverse halves run per output.
 * in and every outs[k]: REAL X slabs [x_local][N1][N2] of dfft_local_count reals, exactly as for dfft_plan_create_conv_real.  `in` is
 * read at every execute and left alone unless one outs[k] equals it (allowed: the forward half has consumed `in` before anything is
 * written).  Two equal outs entries, a NULL entry, outs == NULL or noutputs outside 1 .. DFFT_CONV_MAX_OUTPUTS: DFFT_EINVAL.
 * Everything dfft_plan_create_conv_real refuses is refused here with the same codes (flags, N0 / N1 not single-pass, N2 not of real form
 * 1, more than 2^31 complex elements per device), every check before the device is queried.
 * dfft_conv_set_filter, dfft_conv_set_kernel, dfft_conv_real_filter_count and dfft_plan_set_scale work on the handle unchanged: one base
 * filter, complex or real, 1/(N0*N1*N2) and the scale folded in.  dfft_execute produces all outputs (DFFT_EINVAL before a base filter is
 * set); dfft_plan_sync, dfft_plan_stream, dfft_plan_destroy, dfft_plan_tune, dfft_kernel_times and the buffer accessors as for
 * dfft_plan_create_conv_real; dfft_stage_times: forward YZ stage, all 1 + K exchanges, the X stage, the sum of the K inverse stages;
 * dfft_plan_describe: "pipeline=conv-real-multi outputs=<K> xconv=fused|multi filter=complex|real|unset width=<Nc> ...".  Execute
 * allocates nothing.  All halves run on one stream, one after another. */
#define DFFT_CONV_MAX_OUTPUTS 8
int dfft_plan_create_conv_real_multi(dfft_plan_t* plan, long long n0, long long n1, long long n2, int dtype, void* in, void* const* outs,
                                     int noutputs, dfft_comm_t comm, int global_idx, int total_devices, unsigned flags);
/* The factors of output k: device pointers to elements of the plan's COMPLEX type, ax of N0, ay of N1 and az of N2/2 + 1 elements.  ay is
 * the whole global vector on every rank; the plan takes its own rows y0 .. y0 + y_local.  NULL means all ones, and before the first call
 * for an output all three of its factors are ones.  The plan keeps private copies (az zero-padded to the plan's width Nc).  Synchronises
 * like dfft_conv_set_filter, may be called between executes and leaves the other outputs alone.  DFFT_EINVAL for a handle that is not a
 * multi-output plan and for k out of range. */
int dfft_conv_set_factors(dfft_plan_t plan, int k, const void* ax, const void* ay, const void* az);

/* Elements the caller's buffers of an r2c plan must hold on device global_idx: *real_count reals on the real side (R2C input / C2R
 * output), *complex_count complex elements on the complex side (R2C output / C2R input) -- the result [y_local][Nh][N0] and, for P > 1,
 * the packed send layout of the forward exchange, which the R2C plan writes into `out` before its result.  Pure host arithmetic. */
int dfft_r2c_counts(long long n0, long long n1, long long n2, int total_devices, int global_idx, long long* real_count,
                    long long* complex_count);
/* plan->bufferDev1, which the reference driver writes directly (fftSpeed3d_c2c.cpp:78). */
void* dfft_plan_buffer1(dfft_plan_t plan);
/* the buffer holding the result after execute (bufferDev2 = out, or in when in-place). */
void* dfft_plan_result(dfft_plan_t plan);
void* dfft_plan_stream(dfft_plan_t plan); /* hipStream_t the plan enqueues on */
/* Diagnostics: the plan's internal hand-over buffer between the passes (NULL when the plan has none) and its size in bytes.
 * No counterpart in the reference (its intermediate is bufferDev1 itself, fft_mpi_3d_api.cpp:497). */
void* dfft_plan_workbuf(dfft_plan_t plan, long long* bytes);
/* fft_mpi_execute_dft_3d_c2c (fft_mpi_3d_api.cpp:181-214).  Collective over all devices of the communicator. */
int dfft_execute(dfft_plan_t plan, unsigned exec_flags);
/* Wait for the plan's stream. */
int dfft_plan_sync(dfft_plan_t plan);
/* Optional plan-time measurement (the FFTW_MEASURE of this library; no counterpart in the reference).  The X pass of a
 * single-GPU plan reads the plan's internal hand-over buffer and writes the result buffer; it runs 5-8 % faster when the two
 * lie in different regions of the device's physical memory (profiles/r03/README.md section 1), which consecutive allocations
 * usually do not.  dfft_plan_tune times that ONE kernel -- seven launches of ~0.7 ms per candidate, no complete transforms --
 * on the current buffer and on fresh allocations of the same size made one after the other and all kept until the end (memory
 * is handed out in runs of 2 ... 36 such allocations that behave alike, so a dense walk cannot step over a run), stops as soon
 * as two candidates differ by 3 % and a second timing of the fastest and the slowest confirms a 3.5 % gap, keeps the fastest and frees
 * everything else.  Bounds: DFFT_TUNE_TRIES candidates and a transient footprint of DFFT_TUNE_MEM_PCT per cent of the FREE device
 * memory -- by default 32 candidates / 25 %, because other plans and processes may share the GPU, and 128 / 70 % when at least 90 % of
 * the device's memory is free, i.e. when this process evidently has the GPU to itself (on some boxes 60+ GiB of consecutive
 * allocations behave alike and the short walk finds no fast buffer: profiles/r04/experiments/tune_check_short_walk.log); worst case
 * about a second at 512^3 fp64.  The probe launches overwrite the result buffer (forward plans) with garbage -- its contents are set
 * aside and put back:
 * call it before the first execute, not between an execute and the use of its result.  A no-op for plans without such a
 * buffer (P > 1, un-fused, natural-order, cache-resident sizes) and with DFFT_TUNE=0.  Results of later executes are
 * bit-identical with and without tuning.  The reference-named wrapper fft_mpi_plan_dft_c2c_3d, distFFTOpt, speed3d_c2c and
 * bench.py all call it for out-of-place plans, so the drop-in CLI times the same configuration as the benchmark. */
int dfft_plan_tune(dfft_plan_t plan);
/* One line of text about how this plan executes: pipeline (fused / unfused / natural), whether the YZ stage is one persistent
 * launch or two launches per cache chunk, the chunk geometry, where the intermediate lives, whether the exchange buffers' rows
 * are rotated, the overlap geometry, and whether dfft_plan_tune has placed the hand-over buffer.  Diagnostics (bench.py puts it
 * in its JSON line); no counterpart in the reference.  buf must hold at least 64 bytes. */
int dfft_plan_describe(dfft_plan_t plan, char* buf, int len);
/* What the last dfft_plan_tune of this plan saw: ms[i] = X-pass kernel time on candidate i (at most max_n are written), *kept =
 * index of the candidate the plan now uses (-1: never tuned), *final_ms = the kept candidate re-timed after the others were
 * freed.  Returns the number of candidates tried.  Any output pointer may be NULL. */
int dfft_plan_tune_report(dfft_plan_t plan, int max_n, double* ms, int* kept, double* final_ms);
/* Multiply the result of every later execute by s (e.g. 1/N for a normalised transform: heFFTe's scale::full, the
 * reference's scale_element pass in 3dmpifft_roc, kernel_func.cpp:102-157).  Folded into the X-pass kernel's store, so it
 * costs no extra pass over the data.  s = 1 (the default) reproduces the reference's un-normalised transforms. */
int dfft_plan_set_scale(dfft_plan_t plan, double s);
/* Stage times of the last forward/backward execute in seconds: t[0..3] = t0..t3 (backward: X, exchange, unpack, YZ),
 * from HIP events on the plan's stream (ASYNC) or host clocks (SYNC_STAGES).  Syncs the stream. */
int dfft_stage_times(dfft_plan_t plan, double t[4]);
/* Durations in seconds of the three FFT kernels of the last ASYNC execute of a fused plan: t[0] = Z rows, t[1] = Y columns
 * (+pack), t[2] = X columns (+transpose); HIP events on the plan's stream.  Used for the roofline figures. */
int dfft_kernel_times(dfft_plan_t plan, double t[3]);
/* fft_mpi_destroy_plan (fft_mpi_3d_api.cpp:143-179). */
int dfft_plan_destroy(dfft_plan_t plan);

/* ---- batched 1D building block (the kernels behind t0/t3; templateFFT batchTest-style checks) ---------------------------
 * Buffer contract of dfft_fft1d_rows, dfft_fft1d_cols, dfft_fft1d_any and dfft_fft2d_batch: any element-aligned pointers (fp32 column
 * launches whose `in` or `out` is only 8-byte aligned run the scalar float2 kernels instead of the column-pair ones); in place
 * (out == in) or out of place; byte ranges that overlap only partly: DFFT_EINVAL, checked before the device is queried; with out != in,
 * `in` is never written (the four-step and Bluestein forms work through scratch); nothing outside the batch * n (* width) elements of
 * `out` is written; batch == 0 writes nothing and returns DFFT_OK.
 * Lines are independent in all four: no row, column or plane shares arithmetic with another, so a line of NaN, of zeros or of any
 * magnitude leaves every other line of the batch bit-identical, and nothing outside `in` that is read reaches a result.
 * In-place or out-of-place length-n C2C FFT of `batch` contiguous rows (stride n). */
int dfft_fft1d_rows(void* in, void* out, long long n, long long batch, int dtype, int direction, void* stream);
/* Length-n FFT down the columns of a [n][width] row-major matrix, `batch` matrices back to back.
 * SUPPORTED EXTENT of the column transforms (this statement holds for dfft_fft1d_cols, dfft_fft1d_any and the inner transforms of
 * dfft_rfft1d_strided / dfft_r2r1d_strided; beyond it: DFFT_EUNSUPPORTED, before the device is queried and before scratch is leased).
 * The batch has no limit beyond memory and 2^31 tiles per launch (tile bases are 64-bit).  Inside ONE matrix the tuned kernels keep a
 * thread's offsets in 32 bits, counted in kernel units of w columns: w = width for fp64 (16 bytes) and for fp32 of odd width or with a
 * pointer that is only 8-byte aligned (8 bytes), w = width / 2 for fp32 column pairs (16 bytes).  A pass of n' points over w units is
 * served iff (n' - 1) * w + 63 < 2^32, and width <= 2^31 - 64 always:
 *   - tuned single-pass n (the plan table, <= 4096): the one pass (n, width);
 *   - run-time-scheduled n (other 7-smooth n <= 4096): 64-bit offsets, no further limit;
 *   - four-step n = N1 * N2 (> 4096): pass A (N1, N2 * width) from `in` into the 16-byte-aligned scratch -- pairs iff `in` is aligned --
 *     and pass B (N2, width) on the scratch;
 *   - Bluestein n along [n][s], s > 1: one launch iff n <= 2048 and n * s < 2^31; else the M-point passes in place on the scratch:
 *     (M, s) for M <= 4096, the four-step rule of (M, s) above that.  With M >= 2n - 1 this serves, past n * s = 2^31, fp32 with even
 *     s up to about M * s < 2^33 and nothing in fp64 or with odd s.  A one-launch call of 2^31 or more rows or column tiles: split the batch.
 * dfft_cols_extent_supported / dfft_fft1d_any_extent_supported are this rule. */
int dfft_fft1d_cols(void* in, void* out, long long n, long long width, long long batch, int dtype, int direction,
                    void* stream);
/* 1 when dfft_fft1d_cols accepts [n][width] columns of `dtype`; pairs != 0: both pointers are 16-byte aligned. */
int dfft_cols_extent_supported(long long n, long long width, int dtype, int pairs);
/* 1 when dfft_fft1d_any accepts [batch][n][s] of `dtype`, for every kind of n; in16 / out16 != 0: that pointer is 16-byte aligned. */
int dfft_fft1d_any_extent_supported(long long n, long long s, int dtype, int in16, int out16);

/* Length-n C2C FFT along the middle axis of data[batch][n][s] (s = 1: contiguous rows), unnormalised, in place (out == in) or out of
 * place, for ANY n of kind 1, 2 or 3 (dfft_length_kind).  Kinds 1 and 2 run exactly what dfft_fft1d_rows (s = 1) / dfft_fft1d_cols
 * run (bit-identical results).  Kind 3 runs Bluestein's chirp-z algorithm (csrc/dfft_bluestein.hip): for n <= 2048 one launch that
 * keeps the padded M-point transforms in registers and LDS (the HBM traffic of an n-point transform), above that a multi-pass form on
 * the four-step transforms with scratch from the same per-(device, stream) buffer the four-step lengths use.  The chirp and B^ tables
 * are built on the first call for (device, n, dtype, direction) and cached; dfft_trim frees them and the scratch.
 * DFFT_BLUESTEIN_FUSED=0 (read per call) runs the multi-pass form for n <= 2048 as well (A/B and measurement switch), and so does a
 * column call with n * s >= 2^31 (the one-launch kernel keeps an item's offsets in 32 bits) where the M-point passes can serve it: see
 * SUPPORTED EXTENT at dfft_fft1d_cols.  dfft_bluestein_fused_applies tells the form, dfft_fft1d_any_extent_supported whether the call
 * is served. */
int dfft_fft1d_any(void* in, void* out, long long n, long long s, long long batch, int dtype, int direction, void* stream);
int dfft_bluestein_fused_applies(long long n, long long s);
/* The one-launch rules of dfft_rfft1d_strided (s > 1) and dfft_r2r1d_strided (vec: s even and both pointers aligned to two reals); 0: the
 * composed / multi-pass route in batch chunks.  Both send n * s >= 2^31 (s > 1) to that route. */
int dfft_rfft_cols_fused_applies(long long n, long long s, int dtype);
int dfft_r2r_fused_applies(long long n, long long s, int dtype, int kind, int vec);
/* Scratch bytes the call leases from the per-(device, stream) buffer dfft_trim frees (0: none, or a call beyond the supported extent,
 * which leases nothing; no device is queried).  Batch chunks keep
 * the Bluestein multi-pass, real-column and r2r composed routes at max(256 MiB, one item's) of packed data plus the inner transform's own
 * scratch; a four-step dfft_fft1d_any takes as much as its data.
 *
 * THE CHUNK CAP.  Every "max(256 MiB, one row's / item's / pair's)" in this header is max(cap, one unit's): the cap is 256 MiB unless the
 * environment variable DFFT_SCRATCH_CHUNK_BYTES holds a positive number of bytes (unset, empty or non-positive: 256 MiB).  It is a test
 * and measurement switch -- it makes several chunks of a small problem -- and changes no result beyond the order in which the accumulating
 * routes (dfft_rxspec1d_long, fused) add their chunks.  dfft_stft1d / dfft_istft1d and dfft_rcsd1d look at DFFT_STFT_CHUNK_BYTES and
 * DFFT_RCSD_CHUNK_BYTES first, then at the general name.  A chunk never holds fewer than one unit, nor fewer than a route's own minimum.
 * A plan-less call and each *_scratch_bytes query read the cap ONCE per call, so a query made under the environment of the call it
 * describes announces that call's lease, and nested chunkings (an r2r or paired-row chunk with Bluestein chunks inside, the long routes'
 * rows) cut by one value.  A PLAN reads the cap when it is CREATED: its any-length real rows and Bluestein axes size their plan-owned
 * scratch by it and every execute cuts by that scratch, whatever the variable holds then.  Results of plans do not depend on it. */
unsigned long long dfft_fft1d_any_scratch_bytes(long long n, long long s, long long batch, int dtype);
unsigned long long dfft_rfft1d_strided_scratch_bytes(long long n, long long s, long long batch, int dtype);
unsigned long long dfft_r2r1d_strided_scratch_bytes(long long n, long long s, long long batch, int dtype, int kind, int vec);

/* Real transforms of `batch` contiguous rows, for ANY n with dfft_real_form(n) != 0.  Forward: reals [batch][n] -> bins [batch][n/2+1]
 * (= numpy.fft.rfft).  Backward: bins -> reals, = n * numpy.fft.irfft(row, n) for ANY input (the imaginary parts of bin 0 and, n even,
 * bin n/2 are ignored).  Unnormalised, out of place (the byte ranges of in and out must not overlap: DFFT_EINVAL), `in` is never
 * written.  Form 1 runs the half-length kernels of the r2c plans; forms 2 and 3 pair rows 2p and 2p + 1 in one n-point complex
 * transform (an odd last row is paired with a zero row, or its partner's output dropped), so each row's rounding error is bounded
 * relative to its pair's combined magnitude.  Nothing else is shared: form 1 rows are independent, and in forms 2 and 3 a row of NaN
 * or of any magnitude reaches its partner and no other row (every row outside the pair stays bit-identical).  Scratch and Bluestein
 * tables come from the caches dfft_trim frees. */
int dfft_rfft1d(void* in, void* out, long long n, long long batch, int dtype, int direction, void* stream);

/* Real transforms along the middle axis of [batch][n][s] (s = 1: dfft_rfft1d, bit-identical), for ANY n of dfft_length_kind 1, 2 or 3.
 * Forward: reals [batch][n][s] -> bins [batch][n/2+1][s] (= numpy.fft.rfft(x, axis=1)).  Backward: bins -> reals, = n * numpy.fft.irfft(X, n,
 * axis=1) for ANY input (the imaginary parts of bin 0 and, n even, bin n/2 are ignored).  Unnormalised, out of place (overlapping byte
 * ranges of in and out: DFFT_EINVAL), `in` is never written; any s >= 1 and any element-aligned pointers.  Real columns 2c and 2c + 1 share
 * one n-point complex transform down the column pair (an odd last column is paired with a zero column), so each column's rounding error
 * is bounded relative to its pair's combined magnitude.  Pairs never span two [n][s] items, and a column of NaN or of any magnitude
 * reaches its partner and no other column.  Tuned single-pass n (n * s < 2^31) run as one launch; every other n in batch
 * chunks on the four-step / Bluestein / run-time-scheduled transforms with scratch from the caches dfft_trim frees.  Arguments are checked
 * before the device is queried. */
int dfft_rfft1d_strided(void* in, void* out, long long n, long long s, long long batch, int dtype, int direction, void* stream);

/* Batched 2-D real transforms of `batch` planes [n1][n2] (n2 contiguous), for n2 of any dfft_real_form != 0 and n1 of any
 * dfft_length_kind != 0.  Forward: reals [batch][n1][n2] -> bins [batch][n1][n2/2+1] (= numpy.fft.rfft2).  Backward: n1*n2 *
 * numpy.fft.irfft2(X, s=(n1, n2)) for ANY input (inverse C2C along n1, then C2R along n2 with numpy's rule for the imaginary parts).
 * Unnormalised, out of place (overlap: DFFT_EINVAL), `in` is never written.  Planes are processed in groups sized for the 256 MiB
 * Infinity Cache: R2C rows (dfft_rfft1d) then the n1-point columns in place on `out` (dfft_fft1d_any); backward the inverse columns
 * into a scratch group, then C2R rows into `out`.  Arguments are checked before the device is queried.
 * WHICH PLANES SHARE ARITHMETIC: the rows of a plane group -- all `batch` planes while their bins fit 256 MiB, else the evened chunk of
 * planes dfft_fft2d_batch takes -- go through dfft_rfft1d's row transform as ONE batch of planes_in_group * n1 rows.  n2 of real form 1,
 * or even n1: planes are independent.  n2 of form 2 or 3 with odd n1: rows 2p and 2p + 1 of that flattened batch pair up, so the last
 * row of the group's plane 2q shares a transform with the first row of its plane 2q + 1 (the last row of an odd last plane goes with
 * zeros), and each of the two planes' rounding error is bounded relative to their combined magnitude.  Forward the column pass spreads
 * what crosses over the whole neighbouring plane (a NaN plane makes its partner plane NaN throughout); backward only over that one row.
 * No other plane is reached, in either direction. */
int dfft_rfft2d_batch(void* in, void* out, long long n1, long long n2, long long batch, int dtype, int direction, void* stream);

/* Real-to-real transforms along the middle axis of reals [batch][n][s] (s = 1: contiguous rows), for ANY n of dfft_length_kind 1, 2 or 3
 * (n = 1 included).  Unnormalised, scipy.fft's norm=None and FFTW's REDFT10 / REDFT01 / RODFT10 / RODFT01:
 *   DFFT_R2R_DCT2  y[k] = 2 sum_j x[j] cos(pi k (2j+1) / 2n)
 *   DFFT_R2R_DCT3  y[j] = x[0] + 2 sum_{k>=1} x[k] cos(pi k (2j+1) / 2n)
 *   DFFT_R2R_DST2  y[k] = 2 sum_j x[j] sin(pi (k+1) (2j+1) / 2n)
 *   DFFT_R2R_DST3  y[j] = (-1)^j x[n-1] + 2 sum_{k<n-1} x[k] sin(pi (k+1) (2j+1) / 2n)
 * so type III of type II is 2n x.  Types I and IV are NOT built.  dtype DFFT_F64 (double) or DFFT_F32 (float).  Out of place or exactly
 * in place (out == in); byte ranges that overlap only partly: DFFT_EINVAL; with out != in, `in` is never written.  Any s >= 1 and any
 * element-aligned pointers.  Adjacent columns 2c, 2c + 1 (s > 1) or rows 2p, 2p + 1 (s = 1) share one n-point complex transform (an odd
 * last one is paired with zeros), so each one's rounding error is bounded relative to its pair's combined magnitude; column pairs never
 * span two [n][s] items, and nothing reaches a line outside the pair.  Tuned single-pass
 * n (for s > 1: n * s < 2^31) run as ONE launch that moves the field once in and once out (csrc/dfft_r2r.hip); every other n, and every n
 * under DFFT_R2R_FUSED=0 (read per call), runs pre kernel -> n-point transform -> post kernel in batch chunks.  Scratch, the quarter-wave
 * tables and the Bluestein tables come from the caches dfft_trim frees; a call allocates nothing once they are warm.  Arguments are
 * checked before the device is queried. */
#define DFFT_R2R_DCT2 0
#define DFFT_R2R_DCT3 1
#define DFFT_R2R_DST2 2
#define DFFT_R2R_DST3 3
int dfft_r2r1d_strided(void* in, void* out, long long n, long long s, long long batch, int dtype, int kind, void* stream);

/* Batched 1-D real FFT convolution: every contiguous row of reals in [batch][channels][n] filtered by its channel's spectrum
 * h [channels][m/2 + 1],
 *     out[b, c, :] = numpy.fft.irfft(numpy.fft.rfft(in[b, c, :], m) * h[c, :], m)[:n]        (row r uses filter row r % channels)
 * normalised like the spectral-filter plans (h == 1 gives out == in).  m == n is the circular convolution; m >= n + taps - 1 gives the
 * first n samples of the linear convolution with a kernel of `taps` taps (h = rfft of the zero-padded taps).  Like dfft_rfft1d backward,
 * the imaginary parts of the products at bins 0 and m/2 are ignored.  dtype DFFT_F64 (double) or DFFT_F32 (float); filter_kind
 * DFFT_FILTER_COMPLEX (h holds elements of the complex type) or DFFT_FILTER_REAL (elements of the real type, half the filter bytes).
 * Accepted: 1 <= n <= m, dfft_real_form(m) == 1 (m even, m/2 a single-pass length, so m <= 8192; dfft_rconv1d_length(a) is the smallest
 * such m >= a, 0 if none), channels >= 1, batch >= 1, batch * channels < 2^31 rows (row bases are 64-bit); any element-aligned pointers.
 * Longer sequences run block by block through dfft_rconv1d_os below (overlap-save); four-step and Bluestein halves are NOT built.  Every other m: DFFT_EUNSUPPORTED (and 2^31 or more rows: split the
 * batch); NULL pointers, sizes below 1, m < n, a bad dtype or filter kind, in and out overlapping partly, h overlapping out:
 * DFFT_EINVAL -- all decided before the device is queried.  out == in (exactly) is allowed; with out != in, `in` is never written; h is
 * never written; nothing outside the batch * channels * n reals of out is written.  Rows are independent (no pairing, on either route): a
 * row of NaN or of any magnitude leaves every other row bit-identical, and filter row c reaches exactly the rows of channel c.
 * Where m/2 has a tuned plan the call is ONE launch (csrc/dfft_rconv.hip) that loads the n reals of a row, runs the forward m/2-point
 * transform, splits, multiplies, merges and runs the inverse in registers and LDS, and stores n reals: the row is read once and written
 * once, the zero padding and the spectrum never exist in memory.  Every other accepted m, the few (m/2, dtype) whose kernels would spill
 * or measured slower, and every m under DFFT_RCONV_FUSED=0 (read per call) run pad -> R2C rows -> multiply -> C2R rows -> truncate in
 * batch chunks of at most max(256 MiB, one row's) scratch from the per-(device, stream) buffer dfft_trim frees; a call allocates nothing
 * once that is warm.  dfft_rconv1d_fused_applies tells the route (vec: n even and both pointers aligned to two reals -- the one-launch
 * kernel then moves two reals per access; the route itself does not depend on it), dfft_rconv1d_scratch_bytes the lease (0 for the one
 * launch, and for a call that is refused).  Both are host arithmetic. */
int dfft_rconv1d(const void* in, void* out, const void* h, long long n, long long m, long long channels, long long batch, int dtype, int filter_kind,
                 void* stream);
int dfft_rconv1d_fused_applies(long long n, long long m, int dtype, int filter_kind, int vec);
unsigned long long dfft_rconv1d_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype);
long long dfft_rconv1d_length(long long at_least);

/* Batched 1-D real cross-spectrum, summed over the batch: x and g are rows of reals [batch][channels][n] as in dfft_rconv1d,
 *     out[c, k] = sum_b conj(numpy.fft.rfft(x[b, c, :], m)[k]) * numpy.fft.rfft(g[b, c, :], m)[k],     k = 0 ... m/2,
 * out [channels][m/2 + 1] of the complex type, unnormalised.  It is the filter gradient of dfft_rconv1d (g the gradient of its output;
 * the input gradient is dfft_rconv1d itself with the conjugated filter), and the Welch / cross-spectral-density / matched-filter
 * accumulation; g == x (exactly) is allowed and gives the auto-spectrum sum_b |X|^2.  The imaginary parts of out[c][0] and out[c][m/2]
 * are stored as exact zeros (and every imaginary part of the auto-spectrum).  dtype DFFT_F64 (double) or DFFT_F32 (float).
 * Accepted: the sizes of dfft_rconv1d -- 1 <= n <= m, dfft_real_form(m) == 1 (so m <= 8192), channels >= 1, batch >= 1,
 * batch * channels < 2^31 rows; any element-aligned pointers.  Every other m: DFFT_EUNSUPPORTED (and 2^31 or more rows: split the
 * batch and add the results); NULL pointers, sizes below 1, m < n, a bad dtype, out overlapping x or g: DFFT_EINVAL -- all decided
 * before the device is queried.  x and g are never written; nothing outside the channels * (m/2 + 1) elements of out is written.  A row
 * (b, c) reaches every bin of out[c] and nothing of any other channel.
 * The result is the same bits from call to call: no floating-point atomics.  The batch is cut into dfft_rxspec1d_slices contiguous
 * ranges, the first batch % slices of them one row longer -- host arithmetic on fixed constants, never on the device that is present:
 * slices = max(1, min(target / channels, batch / 8)), target = 512 * min(G, 8) items with G the thread groups per workgroup of the
 * m/2-point kernel (about the resident thread groups of a 256-CU part; G = 1 where m/2 has no tuned plan), so a slice holds at least 8
 * rows -- each slice is summed in row order and the slices are added in slice order, all in the working precision.
 * Where m/2 has a tuned plan the call is ONE launch (csrc/dfft_xspec.hip), plus a small one that adds the slices where there are
 * several: a thread group per (slice, channel) loads the n reals of a row of x, runs the forward m/2-point transform and forms the
 * row's bins in registers, does the same for g, and accumulates the products in registers -- each row of either field is read once
 * and nothing is written per row.  Every other accepted m, the few (m/2, dtype) whose kernels would spill or measured slower, and every
 * m under DFFT_RXSPEC_FUSED=0 (read per call) run pad -> R2C rows on both fields -> a multiply-accumulate in row order, in chunks of
 * rows of at most max(256 MiB, one row's) scratch from the per-(device, stream) buffer dfft_trim frees; a call allocates nothing once
 * that is warm.  dfft_rxspec1d_fused_applies tells the route (vec: n even and both fields aligned to two reals; the route does not
 * depend on it), dfft_rxspec1d_scratch_bytes the lease (the partial sums of the slices, 0 for one slice; the chunk on the composed
 * route; 0 for a call that is refused), dfft_rxspec1d_slices the slice count (0 for sizes that are refused).  All three are host
 * arithmetic. */
int dfft_rxspec1d(const void* x, const void* g, void* out, long long n, long long m, long long channels, long long batch, int dtype, void* stream);
int dfft_rxspec1d_fused_applies(long long n, long long m, int dtype, int vec);
unsigned long long dfft_rxspec1d_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype);
long long dfft_rxspec1d_slices(long long m, long long channels, long long batch, int dtype);

/* Overlap-save form of dfft_rconv1d for rows of ANY length: in [batch][channels][n], out [batch][channels][n_out], h [channels][m/2 + 1]
 * as above.  m is the block length and `discard` (d) the samples dropped per block; with S = m - d and nb = ceil(n_out / S), block b of
 * row r is
 *     xb[i]           = in[r, b S - d + i]  if 0 <= b S - d + i < n, else 0                        (0 <= i < m)
 *     cb              = numpy.fft.irfft(numpy.fft.rfft(xb, m) * h[r % channels], m)                (h == 1 gives cb == xb)
 *     out[r, b S + j] = cb[d + j]                                                                  (0 <= j < S, b S + j < n_out)
 * With h = rfft of `taps` <= d + 1 taps zero-padded to m, out[r] = numpy.convolve(in[r], k)[:n_out]: n_out = n is the causal head,
 * n_out = n + taps - 1 the full convolution.  The imaginary parts of the products at bins 0 and m/2 are ignored.
 * Accepted: n >= 1, 1 <= n_out <= n + discard, dfft_real_form(m) == 1, 0 <= discard <= m - 1, channels, batch >= 1, batch * channels * nb
 * < 2^31 block items (element offsets are 64-bit); any element-aligned pointers.  NULL pointers, sizes out of range, a bad dtype or
 * filter kind, in and out overlapping AT ALL (blocks read what their neighbours write: there is no in-place form), h overlapping out:
 * DFFT_EINVAL; every other m, and 2^31 or more items: DFFT_EUNSUPPORTED -- all decided before the device is queried.  in and h are never
 * written; nothing outside the batch * channels * n_out reals of out is written.  Rows are independent; inside a row a sample reaches
 * the results of the blocks that read it (a NaN at in[r, j] makes at least out[r, j ... j + discard] NaN, and may spread over those blocks).
 * Where m/2 has a tuned plan the call is ONE launch (csrc/dfft_osconv.hip): the kernel of dfft_rconv1d run per (row, block) item with the
 * load base, the store window and the filter row taken from the item -- the padded blocks, the dropped samples and the spectrum never
 * exist in memory; two reals per access where n, n_out and discard are even and both pointers are aligned to two reals.  Every other
 * accepted m, the (m/2, dtype) dfft_rconv1d routes, and every m under DFFT_RCONV_FUSED=0 (read per call) run gather -> R2C rows ->
 * multiply -> C2R rows -> scatter in chunks of items of at most max(256 MiB, one item's) scratch from the buffer dfft_trim frees; a call
 * allocates nothing once that is warm.  dfft_rconv1d_os_fused_applies tells the route, dfft_rconv1d_os_scratch_bytes the lease (0 for the
 * one launch, and for sizes that are refused).  dfft_rconv1d_os_block chooses the block for `taps` taps and n_out results per row:
 * discard = taps - 1 rounded up to even, and the accepted m > discard with the smallest ceil(n_out / (m - discard)) * t(m) over a table of
 * per-block times (one block where one fits); DFFT_EUNSUPPORTED for taps > 8191.  All three are host arithmetic. */
int dfft_rconv1d_os(const void* in, void* out, const void* h, long long n, long long n_out, long long m, long long discard, long long channels,
                    long long batch, int dtype, int filter_kind, void* stream);
int dfft_rconv1d_os_fused_applies(long long m, int dtype);
unsigned long long dfft_rconv1d_os_scratch_bytes(long long n_out, long long m, long long discard, long long channels, long long batch, int dtype);
int dfft_rconv1d_os_block(long long taps, long long n_out, int dtype, long long* m, long long* discard);

/* dfft_rconv1d for padded lengths beyond 8192 -- taps about as long as the row ("long convolution"): the same definition, normalisation
 * and DC / Nyquist rule,
 *     out[b, c, :] = numpy.fft.irfft(numpy.fft.rfft(in[b, c, :], m) * H[c, :], m)[:n]        (row r uses filter row r % channels)
 * with the filter handed over as hp = dfft_rconv1d_long_filter(H): a pure permutation of H [channels][M + 1], M = m/2 = N1 * N2,
 *     hp[c][k1 * N2 + k2] = H[c][k1 + N1 * k2]   (k1 < N1, k2 < N2),        hp[c][M] = H[c][M],
 * of the same element type (hp must not overlap h), which is the order the kernels read coalesced.
 * Accepted: 1 <= n <= m, m even, 8192 < m <= 2^23, M = N1 * N2 with both factors tuned single-pass lengths out of { 2^a, 3 * 2^a, 5 * 2^a
 * in [64, 2048], 81, 125 }; the split is the most balanced such pair with N1 <= N2 (dfft_rconv1d_long_split: 1 and the pair, or 0;
 * dfft_rconv1d_long_length(a): the smallest accepted m >= a, 0 if none).  channels >= 1, batch >= 1, batch * channels < 2^31 rows; any
 * element-aligned pointers.  Every other m: DFFT_EUNSUPPORTED (and 2^31 or more rows: split the batch); NULL pointers, sizes below 1,
 * m < n, a bad dtype or filter kind, in and out overlapping partly, hp overlapping out: DFFT_EINVAL -- all decided before the device is
 * queried.  out == in (exactly) is allowed; with out != in, `in` is never written; hp is never written; nothing outside the
 * batch * channels * n reals of out is written.  On the three-launch route rows are independent (its per-pair step pairs scratch rows
 * of ONE input row); on the composed route below rows 2p and 2p + 1 of the batch * channels rows share their transforms, as in
 * dfft_rfft1d's real form 3, and each row's rounding error is bounded relative to its pair's combined magnitude.
 * Bluestein halves and strided rows are NOT built.  Gradients: the input gradient is this call with the conjugated filter, the filter
 * gradient dfft_rxspec1d_long below.
 * The call is THREE launches per chunk of rows (csrc/dfft_lconv.hip), the fused kernel of dfft_rconv1d cut along the four-step
 * decomposition: N1-point columns read straight from the reals (times the four-step twiddle) into M complex of scratch per row; per pair
 * of scratch rows the N2-point transform, the split / multiply / merge step and the N2-point inverse, in place; the inverse N1-point columns
 * stored as the first n reals -- 2 n + 4 m reals of traffic per row; the zero padding, the spectrum and the truncated tail never exist in
 * memory.  Chunks hold at most max(256 MiB, one row's) scratch from the per-(device, stream) buffer dfft_trim frees; a call allocates
 * nothing once that and the small twiddle tables of (device, m, dtype) are warm.  The splits whose kernels would spill or measured slower,
 * and every m under DFFT_RCONV_LONG_FUSED=0 (read per call), run pad -> the real rows of length m as dfft_rfft1d runs them -> multiply ->
 * inverse rows -> truncate, in chunks of WHOLE ROW PAIRS (an even number of rows, at least two, unless the chunk is the whole call) within
 * max(256 MiB, one pair's) bins and padded rows, so that rows 2p and 2p + 1 are partners wherever the chunks are cut.
 * dfft_rconv1d_long_fused_applies tells the route; dfft_rconv1d_long_scratch_bytes the lease of the three-launch
 * route: min(rows, rows per chunk) * M complex (0 for sizes that are refused; the composed route leases its bins, padded rows and the
 * transforms' own scratch instead).  Both, the length and the split are host arithmetic. */
long long dfft_rconv1d_long_length(long long at_least);
int dfft_rconv1d_long_split(long long m, int* n1, int* n2);
int dfft_rconv1d_long_filter(const void* h, void* hp, long long m, long long channels, int dtype, int filter_kind, void* stream);
int dfft_rconv1d_long(void* in, void* out, const void* hp, long long n, long long m, long long channels, long long batch, int dtype, int filter_kind,
                      void* stream);
int dfft_rconv1d_long_fused_applies(long long m, int dtype);
unsigned long long dfft_rconv1d_long_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype);

/* dfft_rxspec1d for the padded lengths of dfft_rconv1d_long (the filter gradient of that convolution): the same definition,
 *     out[c, k] = sum_b conj(numpy.fft.rfft(x[b, c, :], m)[k]) * numpy.fft.rfft(g[b, c, :], m)[k],        out [channels][m/2 + 1] complex,
 * unnormalised, the imaginary parts of bins 0 and m/2 exact zeros, g == x (exactly) the auto-spectrum with exact-zero imaginary parts
 * throughout.  order 0 stores the bins in natural order; order 1 in the order of dfft_rconv1d_long_filter (out[c][k1 * N2 + k2] =
 * S[c][k1 + N1 * k2], out[c][M] = S[c][M]).  Accepted m: exactly those of dfft_rconv1d_long_split; 1 <= n <= m, channels >= 1, batch >= 1,
 * batch * channels < 2^31 rows.  Every other m: DFFT_EUNSUPPORTED (and 2^31 or more rows: split the batch); NULL pointers, sizes below 1,
 * m < n, a bad dtype or order, out overlapping x or g: DFFT_EINVAL -- all decided before the device is queried.  x and g are never written.
 * Fused route (csrc/dfft_lxspec.hip), per chunk of rows: pass A of dfft_rconv1d_long on both fields (one for the auto-spectrum) into
 * M = m/2 complex of scratch per row and field; an accumulating kernel with one item per (slice, channel, pair of scratch rows) that, for
 * every row of its channel and slice in order, runs the N2-point transforms of x and g, forms 2 X[k] and 2 G[k] of its own bins and adds
 * conj(X[k]) G[k] to running sums in registers (nothing is written per row); a reduction over the slices that writes `out` in the requested
 * order -- 2 n + 4 m reals of traffic per row pair.  NO floating-point atomics, and the cuts are host arithmetic on (m, channels, batch,
 * dtype) and fixed constants, never the device:
 *   chunks  the batch * channels rows, in order, in chunks of max(1, min(rows, max(256 MiB, rb) / rb)) rows, rb = 2 * M complex (both
 *           fields; counted so also for the auto-spectrum);
 *   slices  a channel has at most steps = ceil(chunk rows / channels) rows in a chunk; they are cut into
 *           max(1, min(2048 / (channels * ceil(N1 / 2)), steps / 8)) contiguous ranges, the first steps % slices one step longer
 *           (channels * ceil(N1 / 2) items exist with one slice already);
 *   order   rows of a slice in order, then the slices in order (their sum), then the chunks in order (out += the chunk's sum).
 * So every bit of the result is the same from call to call.  A call of one chunk and one slice in order 1 stores straight to out.
 * The splits whose accumulating kernel would keep values in scratch memory (csrc/dfft_lxspec.hip: lxspec_fused_ok), and every m under
 * DFFT_RXSPEC_LONG_FUSED=0 (read per call), run the composed route: pad -> the real rows of length m as dfft_rfft1d runs them, on both
 * fields -> a kernel that adds each channel's rows to out in row order; deterministic as well, in chunks of whole row pairs (as the
 * composed route of dfft_rconv1d_long) of at most max(256 MiB, one pair's) bins and padded rows, and -- the rows being added in row
 * order onto out -- the same bits wherever the chunks are cut.  dfft_rxspec1d_long_fused_applies tells the route; dfft_rxspec1d_long_slices the slice count of the first
 * (the largest) chunk; dfft_rxspec1d_long_scratch_bytes the lease of the fused route: (chunk rows * 2 * M + slices * channels * (M + 1))
 * complex (0 for sizes that are refused; the composed route leases its bins, padded rows and the transforms' own scratch instead).  All
 * three are host arithmetic.  Bluestein halves and strided rows are NOT built (the framed, windowed form is dfft_rcsd1d, m <= 8192). */
int dfft_rxspec1d_long(const void* x, const void* g, void* out, long long n, long long m, long long channels, long long batch, int dtype, int order,
                       void* stream);
int dfft_rxspec1d_long_fused_applies(long long m, int dtype);
unsigned long long dfft_rxspec1d_long_scratch_bytes(long long n, long long m, long long channels, long long batch, int dtype);
long long dfft_rxspec1d_long_slices(long long m, long long channels, long long batch, int dtype);

/* Batched short-time Fourier transform and its inverse (unnormalised, numpy conventions).  Rows of reals in [rows][n], a window win [m]
 * of reals, frames of m reals that advance by hop >= 1, 0 <= pad < m samples of padding in front of every row.  Frame f of row r is
 *     xb[i]        = P(in[r], f hop - pad + i) win[i]                                              (0 <= i < m)
 *     out[r, f, k] = scale numpy.fft.rfft(xb)[k]                  out [rows][frames][m/2 + 1] complex   (out_kind DFFT_STFT_OUT_COMPLEX)
 *     out[r, f, k] = scale^2 |numpy.fft.rfft(xb)[k]|^2            out [rows][frames][m/2 + 1] reals     (out_kind DFFT_STFT_OUT_POWER)
 * where P(row, s) is row[s] inside [0, n) and outside it 0 (pad_mode DFFT_STFT_PAD_ZERO) or the mirrored sample row[-s] / row[2 (n - 1) - s]
 * (DFFT_STFT_PAD_REFLECT, which needs pad < n).  dfft_stft1d_frames is 1 + (n + 2 pad - m) / hop where n + 2 pad >= m, else 0; a call
 * may ask for fewer frames.  With pad = m/2 this is torch.stft(center=True), with pad = 0 center=False; the (bins, frames) order of
 * torch is the transpose of out's last two axes.
 * Accepted: n >= 1, dfft_real_form(m) == 1 (m even, m/2 a single-pass length, so m <= 8192), 1 <= frames <= the count above, rows >= 1,
 * rows * frames < 2^31 items (element offsets are 64-bit); any element-aligned pointers.  NULL pointers, sizes out of range, a bad
 * dtype, pad mode or out kind, reflect padding with pad >= n, in, out and win overlapping: DFFT_EINVAL; every other m, and 2^31 or more
 * items: DFFT_EUNSUPPORTED -- all decided before the device is queried.  in and win are never written; nothing outside out is written.
 * Every (row, frame) is computed on its own: a sample reaches exactly the frames whose support (mirror images included) holds it, and
 * every other frame of every row stays bit-identical; the inverse likewise -- a frame reaches exactly the samples under its support.
 * Where m/2 has a tuned plan the call is ONE launch (csrc/dfft_stft.hip): the thread group of an item reads its frame straight from the
 * row -- two reals per access for whole frames where n, hop and pad are even and `in` is aligned to two reals, else real by real with
 * the zero or mirrored index --, applies the window in registers, transforms, and stores the bins or their squared moduli: the framed
 * copy (m / hop times the signal) never exists in memory.  Every other accepted m, the (m/2, dtype) whose kernel would spill, and every
 * m under DFFT_STFT_FUSED=0 (read per call) run gather-and-window -> R2C rows (-> modulus) in chunks of items of at most max(256 MiB,
 * one item's) scratch from the buffer dfft_trim frees.  dfft_stft1d_fused_applies tells the route, dfft_stft1d_scratch_bytes the lease
 * (0 for the one launch, and for sizes that are refused).
 *
 * dfft_istft1d is the least-squares overlap-add of torch.istft: in [rows][frames][m/2 + 1] complex, out [rows][n] reals with
 * 1 <= n <= (frames - 1) hop + m - pad, inv_env [n] reals shared by all rows (the caller's 1 / sum_f win^2[t + pad - f hop]):
 *     c_f       = m numpy.fft.irfft(in[r, f], m)                     (the imaginary parts of bins 0 and m/2 are ignored)
 *     out[r, t] = inv_env[t] sum_f win[t + pad - f hop] c_f[t + pad - f hop] / m       over the f with 0 <= t + pad - f hop < m
 * Refusals as above (in, out, win and inv_env must not overlap; in, win and inv_env are never written).  Composed only: per chunk of
 * frames C2R rows into scratch (from a copy of the bins where m/2 is untuned), then one thread per output sample sums its at most
 * ceil(m / hop) contributions in ascending frame order -- no atomics, the result does not depend on the chunking.  Chunks hold whole
 * rows where a row fits; a longer row is cut and every cut transforms again the frames its first outputs share with the cut before.
 * dfft_istft1d_scratch_bytes is the lease: chunks of at most max(256 MiB, one item's) -- except that a chunk never holds fewer than the
 * ceil(m / hop) frames one sample sums, which exceeds that only where hop is a few samples and m several thousand.
 * NOT built: a fused inverse, m > 8192 (four-step and Bluestein frames), two-sided output, reflect padding with pad >= n. */
#define DFFT_STFT_PAD_ZERO 0
#define DFFT_STFT_PAD_REFLECT 1
#define DFFT_STFT_OUT_COMPLEX 0
#define DFFT_STFT_OUT_POWER 1
int dfft_stft1d(const void* in, void* out, const void* win, long long n, long long m, long long hop, long long pad, long long frames, long long rows,
                int dtype, int pad_mode, int out_kind, double scale, void* stream);
int dfft_istft1d(const void* in, void* out, const void* win, const void* inv_env, long long n, long long m, long long hop, long long pad, long long frames,
                 long long rows, int dtype, void* stream);
long long dfft_stft1d_frames(long long n, long long m, long long hop, long long pad);
int dfft_stft1d_fused_applies(long long m, int dtype);
unsigned long long dfft_stft1d_scratch_bytes(long long m, long long frames, long long rows, int dtype, int out_kind);
unsigned long long dfft_istft1d_scratch_bytes(long long m, long long frames, long long rows, int dtype);

/* Framed (Welch) 1-D real cross-spectrum: x and g are rows of reals [rows][n], win [m] a window of reals, frames of m reals that advance
 * by hop >= 1 with no padding and no centring -- frame f of a row is its samples [f hop, f hop + m) --
 *     out[r, k] = scale * sum_f conj(numpy.fft.rfft(win * x[r, f hop : f hop + m])[k]) * numpy.fft.rfft(win * g[r, f hop : f hop + m])[k],
 * k = 0 ... m/2, out [rows][m/2 + 1] of the complex type: the sum that scipy.signal.welch / csd / coherence average (detrend=False).
 * frames must be dfft_stft1d_frames(n, m, hop, 0) = 1 + (n - m) / hop >= 1; the samples behind the last whole frame, and for hop > m the
 * samples between frames, are never read.  g == x (exactly) gives the auto-spectrum sum_f |X_f|^2 with every imaginary part an exact
 * zero; the imaginary parts of out[r][0] and out[r][m/2] are exact zeros always.  dtype DFFT_F64 (double) or DFFT_F32 (float).
 * Accepted: dfft_real_form(m) == 1 (m even, m/2 a single-pass length, so m <= 8192), n >= m, rows >= 1, rows (and so rows * slices)
 * and frames below 2^31 each; any element-aligned pointers.  NULL pointers, sizes out of range, a frame count other than the one above, a
 * bad dtype, out overlapping x, g or win: DFFT_EINVAL; every other m, and 2^31 or more rows or frames (split the rows; split a row at a
 * multiple of hop and add the results): DFFT_EUNSUPPORTED -- all decided before the device is queried.  x, g and win are never written;
 * nothing outside the rows * (m/2 + 1) elements of out is written.  A row reaches its own line of out and no other.
 * The result is the same bits from call to call: no floating-point atomics.  The frames of a row are cut into dfft_rcsd1d_slices
 * contiguous ranges, the first frames % slices of them one frame longer -- host arithmetic on fixed constants, never on the device that
 * is present: slices = max(1, min(target / rows, frames / 8)), target = 512 * min(G, 32) items with G the thread groups per workgroup of
 * the m/2-point kernel (G = 1 where m/2 has no tuned plan) -- each slice is summed in frame order and the slices are added in slice
 * order, all in the working precision.
 * Where m/2 has a tuned plan the call is ONE launch (csrc/dfft_csd.hip), plus a small one that adds the slices where there are several:
 * a thread group per (slice, row) reads a frame of x straight from the row -- two reals per access where n and hop are even and both
 * fields are aligned to two reals, else real by real --, applies the window in registers, transforms and forms the frame's bins in
 * registers, does the same for g (g == x has a lighter kernel of its own: one transform, real sums), and accumulates the products in
 * registers.  A row comes from memory once (its overlapping frames are consecutive trips of one thread group) and m/2 + 1 bins are
 * written per row: neither a spectrogram nor a framed copy exists.  Every other accepted m, the (m/2, dtype, auto or cross) whose
 * kernels would spill or measured no faster, and every m under DFFT_RCSD_FUSED=0 (read per call) run, in chunks of frames of at most
 * max(256 MiB, one frame's) scratch (DFFT_RCSD_CHUNK_BYTES, read per call, lowers the cap; the result does not depend on the chunking)
 * from the per-(device, stream) buffer dfft_trim frees: the bins (auto: squared moduli) of the chunk's frames by the frame kernel of
 * dfft_stft1d where that is built, else gather-and-window -> R2C rows, then a multiply-accumulate in frame order.
 * dfft_rcsd1d_fused_applies tells the route (autos: g == x), dfft_rcsd1d_scratch_bytes the lease (the
 * partial sums of the slices, 0 for one slice; the chunk on the composed route; 0 for sizes that are refused), dfft_rcsd1d_slices the
 * slice count (0 for sizes that are refused).  All three are host arithmetic.
 * NOT built: per-frame detrending, median averaging, two-sided output, padding / centring, frames longer than 8192 and a backward form. */
int dfft_rcsd1d(const void* x, const void* g, void* out, const void* win, long long n, long long m, long long hop, long long frames, long long rows,
                double scale, int dtype, void* stream);
int dfft_rcsd1d_fused_applies(long long m, int dtype, int autos);
unsigned long long dfft_rcsd1d_scratch_bytes(long long m, long long frames, long long rows, int dtype, int autos);
long long dfft_rcsd1d_slices(long long m, long long rows, long long frames, int dtype);

/* ---- batched 2D transform (templateFFT's FFTDim = 2 application: initializeFFT, templateFFT.cpp:5767, launched by fftZY,
 * fft_mpi_3d_api.cpp:466-522; component benchmark templateFFT/batchTest/Test_2D.cpp:29-198) ---------------------------------
 * `batch` planes of [n1][n2] complex elements (n2 contiguous), each transformed along both axes, in place (out == in) or out
 * of place (`in` is left untouched).  This is the t0 stage of a 3D plan as an entry point of its own: planes are processed in
 * groups that fit the 256 MiB Infinity Cache (the column pass reads what the row pass wrote from the cache), and the plane
 * shapes the one-launch stage is built for (fp64; n1 = 256 / 512 with n2 = 256 / 512, n1 = 768 with n2 = 512) run as ONE
 * persistent launch per call.  Un-normalised in both directions.  The one-launch form keeps a small control block per (device,
 * stream, plane shape, direction), freed by dfft_trim(); calls on one stream may change batch, direction, placement and dtype
 * freely (a batch change re-zeroes the block on that stream).  A launch that gives up (see dfft_zy.hip) is reported by
 * dfft_fft2d_batch_status() once the stream has been waited for, or else by the next call on that stream, which -- like every
 * later one -- runs on two launches per chunk. */
int dfft_fft2d_batch(void* in, void* out, long long n1, long long n2, long long batch, int dtype, int direction, void* stream);
/* DFFT_EHIP (with a message) if a one-launch stage of dfft_fft2d_batch on (current device, stream) gave up; call it after waiting
 * for the stream.  Each failure is reported once, here or by the next dfft_fft2d_batch call on that stream. */
int dfft_fft2d_batch_status(void* stream);

/* Frees the scratch buffers the 1-D entry points cache per (device, stream) for lengths above 4096 (four-step transforms) and for
 * Bluestein transforms, the cached Bluestein tables (a plan keeps those of its own axes until it is destroyed), the quarter-wave
 * tables of dfft_r2r1d_strided and the control blocks of dfft_fft2d_batch.
 * Buffers in use by a call in progress are left alone.  No counterpart in the reference. */
int dfft_trim(void);

/* The leases of dfft_rfft1d, dfft_rfft2d_batch and dfft_fft2d_batch from that buffer, by the routines' own rules (host arithmetic, no
 * device is queried): the largest single lease of the call -- what the grow-only buffer holds after it -- and 0 for none or for sizes
 * that are refused.  dfft_rfft1d: 0 for real form 1 (forward, and backward with a tuned n/2; else the copy of a chunk's bins), the
 * paired transforms' scratch for forms 2 and 3.  dfft_rfft2d_batch: forward the larger of the row pass's and dfft_fft1d_any's, backward
 * the bins of a plane group plus the larger of the two passes' own.  dfft_fft2d_batch: nothing for single-pass axes (the one-launch
 * stage included), as much as the data where an axis runs four-step. */
unsigned long long dfft_rfft1d_scratch_bytes(long long n, long long batch, int dtype, int direction);
unsigned long long dfft_rfft2d_batch_scratch_bytes(long long n1, long long n2, long long batch, int dtype, int direction);
unsigned long long dfft_fft2d_batch_scratch_bytes(long long n1, long long n2, long long batch, int dtype);

/* TEST HOOKS, not part of the transform interface: the scratch buffer of (current device, stream) as earlier calls left it.  They take the
 * same lease as every plan-less call.  tests/test_gpu_call_mix.py fills the buffer with NaN bit patterns (byte 0xFF: every fp32 and fp64
 * word a NaN) or zeros before a call and shows that the call's result does not depend on it.
 *   dfft_debug_scratch_fill      grows the buffer to at least_bytes by the usual rule (a smaller one is freed behind a stream wait), then
 *                                enqueues a memset of the WHOLE cached buffer with `byte` on `stream`.  DFFT_OK or a DFFT_E* code.
 *   dfft_debug_scratch_capacity  the bytes cached for (current device, stream); 0 when there are none.
 *   dfft_debug_scratch_count     waits for `stream`, copies the buffer to the host and returns how many of its bytes equal `byte`
 *                                (0 with no buffer; a negative DFFT_E* code on failure).
 * Without a device: DFFT_ENOGPU, 0 and DFFT_ENOGPU; none is touched. */
int dfft_debug_scratch_fill(unsigned long long at_least_bytes, int byte, void* stream);
unsigned long long dfft_debug_scratch_capacity(void* stream);
long long dfft_debug_scratch_count(int byte, void* stream);

/* data[i] *= s for `count` complex elements on the device (the 1/N normalisation both transforms leave to the caller;
 * the reference's scale_element kernel, kernel_func.cpp:102-157, used only by 3dmpifft_roc). */
int dfft_scale(void* data, long long count, int dtype, double s, void* stream);

/* ---- tiny TCP rendezvous for multi-process launches without MPI ----------------------------------------------------------
 * Replaces what the reference driver needs from MPI besides moving data (MPI_Comm_rank/size, MPI_Bcast of the RCCL id,
 * MPI_Barrier, MPI_Reduce(MAX), fftSpeed3d_c2c.cpp:18-26,120-124).  Rank/size/address come from the environment:
 * DFFT_RANK/DFFT_WORLD_SIZE/DFFT_MASTER_ADDR/DFFT_MASTER_PORT, else torchrun's RANK/WORLD_SIZE/MASTER_ADDR/MASTER_PORT,
 * else a PMI/OpenMPI launcher's PMI_RANK/PMI_SIZE or OMPI_COMM_WORLD_RANK/SIZE; single process if none is set. */
int dfft_boot_init(void);
int dfft_boot_rank(void);
int dfft_boot_size(void);
int dfft_boot_bcast(void* buf, size_t bytes, int root);
int dfft_boot_barrier(void);
int dfft_boot_allreduce_max(double* v, int n);
int dfft_boot_finalize(void);
/* Every wait of the rendezvous is bounded by DFFT_BOOT_TIMEOUT_S (default 180 s, 0 = unbounded): a peer that died or left the
 * collective call sequence yields DFFT_ECOMM naming the collective, the rank waited for and the reason.
 * Diagnostics (no counterpart in the reference, whose MPI calls simply hang): the library keeps the last 256 control-plane
 * events of the process (rendezvous collectives, buffer registrations, exchange rounds, RCCL calls, executes of P > 1 plans).
 * They are printed to stderr with every DFFT_ECOMM / DFFT_ERCCL failure (DFFT_TRACE_ON_ERROR=0: not), on SIGUSR2 together with
 * a native backtrace when DFFT_TRACE_SIGNAL=1 is set, and by this call. */
int dfft_trace_dump(void);

#ifdef __cplusplus
}
#endif
#endif /* DFFT_H */
