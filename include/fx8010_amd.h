/* fx8010_amd.h — C ABI of the MI355X-native batch FX8010 interpreter (libfx8010_amd.so).
 *
 * This is the drop-in boundary for the one hot path this project accelerates: the
 * per-sample instruction loop Klangraum::FX8010::process() of easypx/FX8010-Emulator-Core
 * (reference: source/FX8010.cpp:1023-1249), together with the cold front-end it needs
 * (loadFile, the by-name register API).  The reference has no FFI of its own — its boundary
 * is the public surface of class Klangraum::FX8010 (include/FX8010.h:47-75) — so every entry
 * point below names the class member it replaces.  A header-only C++ class with the
 * reference's exact member names sits on top of this ABI:
 *   fx8010-emulator-core_amd/host/FX8010.h.
 *
 * Two families:
 *   fx_*   one emulated DSP, same call-per-sample convention as the reference class;
 *   fxb_*  N independent DSPs stepping one program in SIMT lockstep on one GPU
 *          ("batch"); fxb_process_block(S) ≡ calling process() S times on each of N objects.
 *
 * All compute runs in a hand-written HIP kernel on gfx950.  There is NO CPU fallback:
 * when no HIP device is usable, fx_create/fxb_create return NULL and fx_last_create_error()
 * says why; a failed launch returns a negative code and fxb_last_error() the text.
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer it passes; the
 * library owns the handle and all device state; a handle is not thread-safe - one thread at a
 * time, as with the reference's objects (include/FX8010.h:162-217: plain members, no lock); calls
 * that reach a multi-device handle from two threads are serialised, not made independent - and
 * distinct handles are independent.  A handle may own a builder thread of its own (code generated
 * ahead of time, FXB_INFO_XLATE_BACKGROUND_BUILDS); the environment's FX_* knobs are read when
 * code is generated: do not change the environment while a handle exists.  Return codes: the reference's own where one exists (noted per
 * function), otherwise 0 = ok and <0 = FX_E_*.
 */
#ifndef FX8010_AMD_H
#define FX8010_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FX_E_NODEVICE (-1) /* no usable HIP device / HIP call failed          */
#define FX_E_NOTREADY (-2) /* no program loaded (reference: getReadyStatus()) */
#define FX_E_ARG (-3)      /* bad argument                                    */
#define FX_E_PROGRAM (-4)  /* program cannot be lowered for the device (see fxb_last_error) */
#define FX_E_MEMORY (-5)   /* device allocation failed                        */

/* Options: behaviour BEYOND the reference, off by default - with every option off the library is the reference, bit for bit.
 * Set before loading a program (fx_set_option / fxb_set_option / fxp_set_option; 0 or FX_E_ARG).
 *
 * FX_OPT_TRAM_DANE  the delay-line model the reference's own design note asks for but does not implement
 *   (docs/TRAM Registermapping.pdf p.1-3; the reference advances a cursor per executed instruction and reads
 *   buf[(rpos - p) % size] with C's remainder, source/FX8010.cpp:909-967, so only offset 0 is defined):
 *     - one address counter per TRAM that steps DOWN once per sample period; a tap, read or write, addresses
 *       (counter + position) mod size (true ring): a value written at position pw is read pr - pw samples later at pr -
 *       any number of taps per delay line, the kX / DANE convention ("idelay write wrt at 0; idelay read rd at 1439");
 *     - the position of "idelay read, rd, at, 17" lives in a register of its own, "&rd" (the PDF's GPR "&rd", created with
 *       the literal as its value), which instructions may name as an operand and write: modulated delay lines;
 *     - no FXO_OOD flag for offsets (there is nothing out of the domain in a ring).
 * FX_OPT_TRAM_ADDR_SHIFT  position registers hold DANE addresses, the "Address-Shifting (0x800)" of the PDF: the FX8010
 *   keeps an address in a register as a 32-bit fixed-point fraction with 0x800 units per sample, so
 *   position = floatToInt(value) >> 11 = floor(value * 2^20) (floatToInt as source/FX8010.cpp:1016-1020), and a tap declared
 *   "at 1439" starts with &rd = 1439 * 2^-20.  That keeps addresses inside [-1, 1): MACS / MACSN / INTERP can compute
 *   them (kX's "macs t, &wrt1, rd_max_shifted, sin_abs"); the low 11 bits (the interpolation fraction) are dropped.
 * Implemented as generated code by the translated tier (taps whose position is the same in every instance), by the HIP C++
 * kernel tier (FXB_INFO_KERNEL 0; also taps with a per-instance position) and, as the checker, by oracle/ (FXO_OPT_*). */
#define FX_OPT_TRAM_DANE (1u << 0)
#define FX_OPT_TRAM_ADDR_SHIFT (1u << 1)
/* FX_OPT_TRAM_INTERP  (with FX_OPT_TRAM_ADDR_SHIFT) the interpolated read the reference's comment asks for ("To do linear
 *   Interpolation, you need to find the fractional part of the read position and interpolate between the two adjacent
 *   samples", source/FX8010.cpp:929-932; ":1192 (Y-2048) mit 11 Bit Shift"): a READ tap at DANE address a = floatToInt(value)
 *   returns x0 + f * (x1 - x0), x0 at position a >> 11, x1 at the position after it, f = (a & 0x7ff) / 2048 - four fp32
 *   operations in that order; f == 0 returns x0 itself.  Writes ignore the fraction. */
#define FX_OPT_TRAM_INTERP (1u << 2)

typedef struct fx_handle fx_handle;   /* one emulated DSP  */
typedef struct fxb_handle fxb_handle; /* a batch of N DSPs */

/* ------------------------------------------------------------------ single instance
 * Mirrors Klangraum::FX8010 one to one (batch of 1 on the current HIP device). */

/* FX8010::FX8010(int numChannels)            include/FX8010.h:51, source/FX8010.cpp:9-12 */
fx_handle* fx_create(int num_channels);
/* FX8010::~FX8010()                          include/FX8010.h:52 */
void fx_destroy(fx_handle* h);
/* bool loadFile(const string& path)          include/FX8010.h:62, source/FX8010.cpp:777-875
 * returns 1 = loaded, 0 = open failure or syntax errors (see fx_error_*). */
int fx_load_file(fx_handle* h, const char* path);
/* vector<float> process(const vector<float>&) include/FX8010.h:57, source/FX8010.cpp:1023-1249
 * in[num_channels] -> out[num_channels], one sample period.  0 or FX_E_*. */
int fx_process(fx_handle* h, const float* in, float* out);
/* S consecutive process() calls in one launch; in/out are [S][num_channels]. */
int fx_process_block(fx_handle* h, const float* in, float* out, int n_samples);
/* int setRegisterValue(const string&, float)  source/FX8010.cpp:236-253: 0 = found, 1 = not found */
int fx_set_register(fx_handle* h, const char* key, float value);
/* float getRegisterValue(const string&)       source/FX8010.cpp:256-266: 1.0f when not found */
float fx_get_register(fx_handle* h, const char* key);
/* int getInstructionCounter()                 source/FX8010.cpp:986-989 (64-bit here) */
int64_t fx_instruction_counter(fx_handle* h);
/* vector<MyError> getErrorList()              include/FX8010.h:63-68, source/FX8010.cpp:894-897
 * entry 0 is always {"Kein Fehler", 1}. */
int fx_error_count(fx_handle* h);
const char* fx_error_desc(fx_handle* h, int i);
int fx_error_row(fx_handle* h, int i);
/* vector<string> getControlRegisters()        source/FX8010.cpp:201-204 */
int fx_control_count(fx_handle* h);
const char* fx_control_at(fx_handle* h, int i);
/* unordered_map<string,string> getMetaData()  source/FX8010.cpp:1003-1006
 * keys name, copyright, created, engine, comment, guid; 1 = present, 0 = absent */
int fx_meta_get(fx_handle* h, const char* key, char* buf, int buflen);
/* setChannels / getChannels / getReadyStatus  include/FX8010.h:73-75 */
void fx_set_channels(fx_handle* h, int num_channels);
int fx_set_option(fx_handle* h, unsigned option, int on);
int fx_get_channels(fx_handle* h);
int fx_ready(fx_handle* h);
const char* fx_last_error(fx_handle* h);
/* why the last fx_create / fxb_create returned NULL (thread-local string) */
const char* fx_last_create_error(void);

/* ------------------------------------------------------------------ batch (the GPU path)
 * N independent instances of one program; instance n of sample s, channel c lives at
 * buf[(s * num_channels + c) * N + n]  — instance-fastest, so a wavefront (64 consecutive
 * instances) reads and writes 256 contiguous bytes. */

/* device: HIP ordinal, or -1 for the calling thread's current device. */
fxb_handle* fxb_create(int64_t n_instances, int num_channels, int device);
/* The same batch spread over several GPUs of one node (SURVEY.md section 8 b/e; the reference's README.md:13 "emulate
 * much more DSP's" on many cores): contiguous instance ranges, whole wavefronts per shard, one host thread + one HIP
 * stream per shard inside the library, program / tables / broadcast controls replicated, NO exchange between shards.
 * Every fxb_* call works on such a handle unchanged (instances keep their global numbers; host PCM buffers keep the
 * [sample][channel][all instances] layout and each shard works on its own columns: in place where the buffers are pinned
 * memory its device can address - fxb_host_alloc asks for memory that every device may map - with staged copies of its
 * columns otherwise);
 * device-resident PCM is per device and goes through fxb_process_block_dev_shards.
 *   fxb_create_sharded     one shard per set bit of device_mask (bit d = HIP ordinal d), in ordinal order
 *   fxb_create_on_devices  one shard per list entry; an ordinal may repeat (several shards on one GPU) */
fxb_handle* fxb_create_sharded(int64_t n_instances, int num_channels, uint64_t device_mask);
fxb_handle* fxb_create_on_devices(int64_t n_instances, int num_channels, const int* devices, int n_devices);
int fxb_shard_count(fxb_handle* h);
/* device ordinal, first global instance and instance count of a shard; 0 or FX_E_ARG.  Any out pointer may be NULL. */
int fxb_shard_info(fxb_handle* h, int shard, int* device, int64_t* first_instance, int64_t* n_instances);
/* HIP-event time of shard `shard`'s most recent launch in ms (fxb_last_kernel_ms is the slowest shard's); -1 when unknown.  A
 * scaling run reports every device with it ("report per-device times too"). */
float fxb_shard_kernel_ms(fxb_handle* h, int shard);
/* The partition fxb_create_sharded / fxb_create_on_devices use for n_instances over n_shards devices, without creating
 * anything (no device needed): first_instance[k], n_instances[k] for k < n_shards.  0, or FX_E_ARG when a shard would be
 * empty (fewer wavefronts than shards) or an argument is invalid. */
int fxb_shard_plan(int64_t n_instances, int n_shards, int64_t* first_instance, int64_t* n_instances_out);
void fxb_destroy(fxb_handle* h);
int fxb_set_option(fxb_handle* h, unsigned option, int on);   /* FX_OPT_*: before loading */
/* as fx_load_file; the program is parsed once on the host and lowered to the device
 * opcode stream.  fxb_load_text takes the program text itself. */
int fxb_load_file(fxb_handle* h, const char* path);
int fxb_load_text(fxb_handle* h, const char* text);
/* setRegisterValue on every instance / on one instance (0 found, 1 not found, <0 FX_E_*) */
int fxb_set_register(fxb_handle* h, const char* key, float value);
int fxb_set_register_i(fxb_handle* h, const char* key, int64_t instance, float value);
/* getRegisterValue of one instance (1.0f when not found) */
float fxb_get_register_i(fxb_handle* h, const char* key, int64_t instance);
/* setRegisterValue / getRegisterValue of every instance at once: values[n_instances], one per instance - what N
 * callers of the reference's setRegisterValue would do before a block (per-instance control automation).
 * 0 found, 1 not found, <0 FX_E_*.  One host-to-device copy; the register becomes per-instance. */
int fxb_set_register_array(fxb_handle* h, const char* key, const float* values);
int fxb_get_register_array(fxb_handle* h, const char* key, float* values);
/* Control track: a schedule of values for register `key` that the NEXT fxb_process_block* call applies by itself - at
 * sample s of that block, whenever s is a multiple of `period`, the register takes values[s / period] (per_instance:
 * values[(s / period) * n_instances + instance]) - exactly what a caller of the reference does with setRegisterValue()
 * between process() calls (the slider every 8 samples of source/main.cpp:107-114), in ONE launch instead of one per
 * change.  At most 16 registers can have tracks (one sorted list of events per block: the loop pays one compare per sample whatever their number); steps beyond the block are dropped; the register keeps its last value.
 * The translated program reads the schedule from device memory (no re-translation per schedule); the interpreter and
 * HIP C++ tiers cut the block at the change points.  0 found, 1 not found, <0 FX_E_*. */
int fxb_set_register_track(fxb_handle* h, const char* key, const float* values, int n_steps, int period, int per_instance);
/* white-noise generator seeds of one instance (reference: g_x1/g_x2, include/FX8010.h:290-291;
 * every instance starts with the reference's seeds) */
int fxb_seed_noise_i(fxb_handle* h, int64_t instance, int32_t x1, int32_t x2);
/* Generate the code blocks of n_samples samples will run, now: the translation (4-9 ms) otherwise falls into the first
 * fxb_process_block* call after a load.  wait != 0: also until the handle's builder thread has finished what follows a first
 * build (the variant with the declared controls in rows; stage counts on trial; the variant for the controls that rest, which
 * is then in force on return: FXB_INFO_CONTROL_ROWS).  For callers with a deadline per block (the
 * reference's caller has 667 us, include/FX8010.h:38): load, prepare, then start the stream.  0 or FX_E_*. */
int fxb_prepare(fxb_handle* h, int n_samples, int wait);
/* State snapshot.  The reference keeps all DSP state in plain members (include/FX8010.h:162-217, 288-291: register values, output
 * latches, smallDelayBuffer / largeDelayBuffer and their four positions, the LFSR words, the instruction counter); a batch's
 * state is the same per instance.  fxb_save_state writes fxb_state_size(h) bytes: a 64-byte header, then - by GLOBAL instance -
 * the state rows [row][instance], iTRAM [instance][slot] and xTRAM [instance][slot] (slots: as many as the program can reach).
 * fxb_load_state takes such an image into a batch of the same instance count with the same program loaded, whatever its
 * partition into shards (a sharded handle can be re-partitioned: save, destroy, create on other devices, load); the registers'
 * host side follows the image (a register every instance holds one value of counts as a broadcast write of that value).
 * Synchronous; 0 or FX_E_*.  Sizes: config5's 262 144 instances carry 8 GiB of xTRAM. */
int64_t fxb_state_size(fxb_handle* h);
int fxb_save_state(fxb_handle* h, void* buf, int64_t cap);
int fxb_load_state(fxb_handle* h, const void* buf, int64_t bytes);
/* Per-instance state: copy, reset, save and load by list.  For a host that treats instances as voices or sweep points: restart a
 * voice, fork a running instance into variants, move a few voices to another handle or GPU, checkpoint the instances it cares
 * about - without the whole-batch image above.  The state of one instance is a RECORD of W = fxb_info(h, FXB_INFO_INSTANCE_WORDS)
 * 32-bit words: the state rows in the order of the whole-batch image (registers, output latches, the four delay-line positions,
 * LFSR words, flags, counter), then the iTRAM slots, then the xTRAM slots - exactly the words fxb_save_state holds for that
 * instance.  An INSTANCE IMAGE is a 64-byte header (the whole-batch header with a magic of its own and the number of records) and
 * `count` records back to back: fxb_instance_image_size(h, count) bytes (FX_E_* below 0).  Lists hold global instance numbers
 * 0..N-1 on any handle, sharded ones included; they are copied before a call returns.  Two HIP kernels move the words as bit
 * patterns (NaN payloads survive) between the transposed state blocks and packed records; records beyond a 64 MiB scratch go in
 * pieces.  All four calls are ordered behind every block queued on the handle so far, on whichever stream, and in front of every
 * later block; they leave meters, armed control tracks and the FXB_INFO_*_BLOCKS counters alone.  FXB_INFO_INSTANCE_GATHERS /
 * _SCATTERS count the kernels' launches.
 *
 * fxb_copy_instances: instance dst[k] becomes a bit-for-bit copy of src[k] - every state row and all delay memory.  A source may
 *   repeat (fan-out); a destination may neither repeat nor appear among the sources.  Stream-ordered: it may return before it has
 *   run, fxb_sync covers it.  On a sharded handle a pair that crosses shards goes through pinned host memory and the call blocks.
 *   What the host knows about the registers does not change (a register it holds as one value is equal in src and dst already).
 * fxb_reset_instances: every listed instance takes the state of a freshly created one - registers at the value of the last
 *   broadcast fxb_set_register (the program's initial value if there was none; per-instance writes to that instance are gone;
 *   the last applied step of a broadcast fxb_set_register_track counts as a broadcast write, per-instance tracks, arrays and
 *   list sets do not),
 *   latches 0, the LFSR at the reference's seeds, flags 0, counter 0, delay memory 0 - EXCEPT the four delay-line positions, which
 *   are kept.  Translated code keeps the positions of a program whose delay-line instructions all run unconditionally in scalar
 *   registers, one set for the wavefront: all instances of such a batch must agree on them.  Kept positions are also what the
 *   signal needs: where every sample period makes as many reads as writes at offset 0 (every program under programs/) only the
 *   distance between the positions matters, and a reset instance produces exactly the outputs of a fresh reference object.  For any
 *   other program the result is "a fresh object whose positions were set to these".  Stream-ordered like the copy.
 * fxb_save_instances: the records of the listed instances (repeats allowed), in list order, behind the header.  Synchronous.
 * fxb_load_instances: the inverse, into any handle with the same program and options - instance count, instance numbers and the
 *   partition into shards may all differ.  Delay-line rule: if the program executes delay-line instructions, the four position
 *   words of every record must equal those its destination holds now, else FX_E_ARG and nothing changes; handles that have run the
 *   same number of samples of the same program satisfy it (migration between handles or GPUs, undo before further processing).
 *   fxb_load_instances_rotated (below) takes records at any position.  A register the host held as one value and that a record
 *   holds another value of becomes per-instance, as if fxb_set_register_i had written it.  Synchronous.
 * 0, FX_E_NOTREADY without a program, or FX_E_ARG with nothing launched and nothing changed: count < 0, a null list with
 * count > 0, an instance outside 0..N-1, a repeated destination, a destination among the sources, a short buffer, an image of
 * another program, kind or version.  count == 0 returns 0. */
int64_t fxb_instance_image_size(fxb_handle* h, int64_t count);
int fxb_copy_instances(fxb_handle* h, const int64_t* src, const int64_t* dst, int64_t count);
int fxb_reset_instances(fxb_handle* h, const int64_t* list, int64_t count);
int fxb_save_instances(fxb_handle* h, const int64_t* list, int64_t count, void* buf, int64_t cap);
int fxb_load_instances(fxb_handle* h, const int64_t* list, int64_t count, const void* buf, int64_t bytes);
/* fxb_load_instances with another delay-line rule: a record loads at ANY position of its destination, its delay memory rotated on
 * the GPU by the difference of the positions (kernel fx_inst_scatter_rot) - undo after further processing, recall of a sounding
 * voice, migration between handles of different age.  Images, lists, image checks, the promotion of registers, ordering (behind
 * every queued block, synchronous) and what is left alone are those of fxb_load_instances.
 *   For each delay line L (iTRAM, xTRAM) the program uses: Z = its size, A = its allocated slots (FXB_INFO_ITRAM_SLOTS /
 *   _XTRAM_SLOTS), (w_s, r_s) the record's write and read position words, (w_d, r_d) those the destination holds now.  L is a RING
 *   when A == Z: in the reference model when every delay write on L has a uniform offset of 0 (every program under programs/), in
 *   the FX_OPT_TRAM_DANE model always.  FXB_INFO_INSTANCE_RINGS tells.
 *   The rotation d of a record on L, in 0..Z-1.  Reference model: d_w = (w_d - w_s) mod Z, d_r = (r_d - r_s) mod Z; a position
 *   kind the program has no instruction of on L (no write, or no read) never moves and does not count (an instruction that is
 *   there counts even if no instance ever executes it: the conservative side, such records are compared rather than trusted); if both count they must
 *   agree and d is that value, if one counts d is its value.  DANE model: d = (w_d - w_s) mod Z (the r words are unused there).
 *   FX_E_ARG, nothing launched, nothing changed, fxb_last_error naming the line and the list entry: a record position word outside
 *   0..Z-1; d_w != d_r (record and destination are in different phases of a program whose reads and writes drift apart, or of a
 *   delay instruction in a SKIP shadow); d != 0 on a line that is not a ring (such a line loads with d = 0, as in fxb_load_instances).
 *   Effect: every state row of the destination takes the record's word - flags included - except the four position rows, which
 *   keep the destination's values (translated code holds one set of positions per wavefront: the neighbours keep agreeing).  On a
 *   ring, slot (j + d) mod Z of the destination takes the record's slot j, j = 0..Z-1, as a 32-bit pattern; a line that is not a
 *   ring is copied as it is.  d may differ between the records of an image and between the two lines of a record.
 *   From the call on the destination produces the outputs, register bits, instruction counter and LFSR words the saved instance
 *   would have produced on the same input, bit for bit; its delay memory is the saved instance's, rotated by d.  One caveat:
 *   out-of-domain flag 1 (FXO_OOD_TRAM_READ_NEG, a read offset beyond the read position) is raised by absolute position, so a
 *   program with read offsets above 0 may raise it at other samples after a rotation - the data is the same, the library defines
 *   that read as the wrapped slot.  With d = 0 everywhere the call leaves exactly the state fxb_load_instances leaves.
 *   A program without delay lines, or one that executes no delay-line instruction, goes the way of fxb_load_instances; otherwise
 *   FXB_INFO_INSTANCE_ROTATIONS counts the launches and FXB_INFO_INSTANCE_SCATTERS does not.  Returns as fxb_load_instances. */
int fxb_load_instances_rotated(fxb_handle* h, const int64_t* list, int64_t count, const void* buf, int64_t bytes);
/* Record banks: instance records kept on the GPU and recalled by list - a note-on from a preset, a checkpoint and its recall, a
 * winner forked into its group after more blocks have run - queued behind the blocks like the other sets by list.  A BANK is
 * n_slots packed records of W = FXB_INFO_INSTANCE_WORDS words in device memory of the handle's GPU, owned by the handle: one bank
 * per handle.  Only the list entries cross PCIe in a store or a recall; no record and no position row does, and neither call waits
 * for a queued block.  Three kernels (fx_bank_gather, fx_bank_rotations, fx_bank_scatter_rot) move the words as bit patterns.
 *
 * fxb_bank_create: a bank of n_slots >= 1 slots, zero-filled; an existing bank is replaced (nothing of it is kept), n_slots == 0
 *   frees it.  FX_E_NOTREADY without a program, FX_E_ARG for n_slots outside 0..2^31-1, FX_E_MEMORY with nothing changed - the old
 *   bank included - when the allocation fails.  A program load (fxb_load_file / fxb_load_text) and fxb_destroy free the bank: its
 *   records are those of the program that was.  fxb_bank_slots: n_slots, 0 without a bank.
 * fxb_bank_store: slot slots[k] takes the record of instance list[k], bit for bit - the words fxb_save_instances would write.
 *   Instances may repeat, slots may not.  Stream-ordered inside the frame of the sets by list: behind every block queued so far on
 *   whichever stream, in front of every later one; fxb_sync covers it.  The only host wait is the frame's own, for the previous
 *   call by list.  On a handle of several shards it blocks (below).
 * fxb_bank_recall: instance list[k] takes the record in slot slots[k] under exactly the rule of fxb_load_instances_rotated - every
 *   state row but the four position rows, the delay memory rotated per record and per line by d, with that call's definition of d,
 *   of a ring and of which position kinds count, the FX_OPT_TRAM_DANE model included.  The DEVICE works out d, from the record's
 *   position words in the bank and the position rows the destination holds when the kernel runs: no position is copied to the
 *   host, nothing is waited for, the call returns 0 once queued.  Slots may repeat (fan-out), destinations may not.  A program
 *   that executes no delay-line instruction takes the plain scatter, position words included.
 *   The three refusals of the rotated load that depend on the record are the device's here: a record position word outside
 *   0..Z-1 (FXB_BANK_BAD_POSITION), d_w != d_r (FXB_BANK_PHASE), d != 0 on a line that is no ring (FXB_BANK_NO_RING).  They are
 *   all or nothing per call: a first small kernel works out the rotations and counts the bad entries into a device cell, the
 *   scatter reads that cell and every workgroup leaves without a store if it is not zero.  A refused recall changes no word of
 *   the batch and still returns 0.  (The host has noted its registers as for a recall that ran: at most a register row more.)
 * fxb_bank_status: waits for the queued bank calls, then reports how many recalls the device has refused since the last reset,
 *   and of the most recent refused one the lowest bad list entry (-1: none) and its reason (FXB_BANK_*; 0: none; an entry bad on
 *   both lines reports iTRAM's).  Any of the three pointers may be null; reset != 0 zeroes the count afterwards.
 * fxb_bank_put / fxb_bank_get: slots from and to the instance-image format above - record k of the image and slot slots[k] - with
 *   the header and the checks of fxb_load_instances / fxb_save_instances (fxb_instance_image_size(h, count) bytes).  Synchronous,
 *   behind everything queued.  A store followed by a get gives the bytes of fxb_save_instances; an image of fxb_save_instances
 *   that is put and recalled leaves what fxb_load_instances_rotated leaves.  put: slots may not repeat; get: they may.  They are
 *   also the door to another handle's bank.
 * Registers: the host keeps, per slot, what it knows of every register that is neither tracked nor kept per instance by the
 *   program itself - the word (a put knows the image's; a store knows the bits of a register the host holds as one value at that
 *   moment) or "unknown".  A recall makes a register per-instance, as if fxb_set_register_i had written it, unless every recalled
 *   slot is known to hold the bits the host holds now: storing and recalling voices whose controls were never moved asks for no
 *   other code (FXB_INFO_NUM_LANE_REGS stays), and a recall across a broadcast fxb_set_register keeps the stored value in the
 *   recalled voice and the broadcast one in the others.
 * Sharded handles: every shard holds its own copy of the bank (FXB_INFO_BANK_BYTES sums them), so any instance recalls any slot
 *   without traffic between devices.  put goes to every shard.  store gathers on the shard that owns the instance and then copies
 *   the stored slots to the other shards through pinned host memory: with more than one shard it blocks, as a crossing pair of
 *   fxb_copy_instances does.  recall is split by shard and stays stream-ordered on each; THE GATE HOLDS PER SHARD - a bad entry
 *   stops the part of the call that fell to its shard, the other shards' parts run - the refused count sums the shards (a call
 *   refused on two shards counts twice) and `entry` is in the caller's numbering: an index into the list as it was passed.
 * Bank calls leave meters, armed control tracks and the FXB_INFO_*_BLOCKS counters alone.  FXB_INFO_BANK_STORES / _RECALLS count
 *   the launches of fx_bank_gather / fx_bank_scatter_rot - a refused recall has launched - and FXB_INFO_INSTANCE_* do not move.
 * 0, FX_E_NOTREADY without a program, or FX_E_ARG with nothing launched, nothing changed and the reason in fxb_last_error: no
 * bank, count < 0, a null list with count > 0, a slot outside 0..n_slots-1, an instance outside 0..N-1, a repeated slot in store
 * or put, a repeated destination in recall, a short buffer, an image of another program, kind or version.  count == 0 returns 0
 * on a handle with a bank. */
#define FXB_BANK_BAD_POSITION 1
#define FXB_BANK_PHASE 2
#define FXB_BANK_NO_RING 3
int fxb_bank_create(fxb_handle* h, int64_t n_slots);
int64_t fxb_bank_slots(fxb_handle* h);
int fxb_bank_store(fxb_handle* h, const int64_t* slots, const int64_t* list, int64_t count);
int fxb_bank_recall(fxb_handle* h, const int64_t* slots, const int64_t* list, int64_t count);
int fxb_bank_put(fxb_handle* h, const int64_t* slots, int64_t count, const void* image, int64_t bytes);
int fxb_bank_get(fxb_handle* h, const int64_t* slots, int64_t count, void* buf, int64_t cap);
int fxb_bank_status(fxb_handle* h, int64_t* refused_calls, int64_t* entry, int* reason, int reset);
/* Register sets by list: the parameters of the program itself - a cutoff, a decay, a pitch per voice - for the instances a host
 * moves, scattered on the GPU behind the queued blocks.  fxb_set_register_i waits on the host for every queued block and copies
 * four bytes; fxb_set_register_array moves all N values of a register.  These two move n_keys * count words with one launch.
 *
 * values[k * count + i] belongs to register keys[k] of global instance list[i]: the [key][entry] order, as the gain lists use
 * [channel][entry].
 * fxb_set_registers_list: afterwards the handle is in exactly the state that n_keys * count calls of
 *   fxb_set_register_i(h, keys[k], list[i], values[k * count + i]) would have left - the words on the device, what the library
 *   knows about the registers, what every get call then returns.  Values are 32-bit patterns: NaN payloads, -0 and denormals
 *   arrive as given and nothing is checked for finiteness (fxb_set_register_i checks nothing either).
 *   Ordering: the call is STREAM-ORDERED.  It runs behind every block queued on the handle so far, on whichever stream - such a
 *   block keeps the values it was queued with - and in front of every block queued later, on whichever stream.  It may return
 *   before it has run; fxb_sync covers it, and so does every call that waits for the queued blocks: fxb_set_register, _i, _array,
 *   the get calls, fxb_save_state, the calls by instance list.  The caller's arrays are free on return.  A second list set behind
 *   the same running block does wait on the host for the first one's scatter (the staging is reused).
 *   Code: as with fxb_set_register_i, the FIRST per-instance write to a register whose value the code in force has folded in asks
 *   for other code, which the next block generates (or finds cached); every later write to that register is a plain scatter.  A
 *   real-time host therefore makes its first list set of every register it will move BEFORE fxb_prepare.
 * fxb_get_registers_list: values[k * count + i] = what fxb_get_register_i(h, keys[k], list[i]) returns, bit for bit.  Synchronous
 *   (it waits for everything queued, a list set included).  A register whose value the library holds once for all instances is
 *   answered without a launch.  Repeated instances and repeated keys are allowed.
 * Returns 0 - also for count == 0 or n_keys == 0, once the keys have been looked up - or, with nothing launched and nothing
 *   changed: FX_E_ARG for a negative count or n_keys, a null keys / list / values with something to do, an instance outside
 *   0..N-1, n_keys * count >= 2^31 and, for the set only, an instance listed twice or two keys that name one register (the order
 *   of two scattered words is undefined); FX_E_NOTREADY without a program; 1 for a key that is no register (fxb_last_error names
 *   it); FX_E_MEMORY when the staging - 2 * count + n_keys * (count + 1) words in device memory and as many pinned, grown on
 *   demand in the call, never inside a block, freed with the handle - could not be allocated, on any shard.
 * Sharded handles: every shard gets the entries that fall to it with their columns of `values`; a shard without one launches
 *   nothing and changes nothing, as with fxb_set_register_i.
 * FXB_INFO_REGISTER_LIST_SETS / _GETS count the launches of the two kernels (fx_reg_scatter, fx_reg_gather). */
int fxb_set_registers_list(fxb_handle* h, const char* const* keys, int n_keys, const int64_t* list, int64_t count, const float* values);
int fxb_get_registers_list(fxb_handle* h, const char* const* keys, int n_keys, const int64_t* list, int64_t count, float* values);
/* Register tracks by list: a change of a program parameter AT A GIVEN SAMPLE of the next block, for the voices a host names - a
 * note-on at sample 13 of a 32-sample block, a glide, an envelope segment for the handful of voices that are moving.  The dense
 * form, fxb_set_register_track(..., per_instance = 1), wants n_steps * N floats from the host, a value for every voice that does
 * not move included; cutting the block and calling fxb_set_registers_list at each cut costs a launch floor per piece.
 *
 * One call arms one LIST SCHEDULE for the next fxb_process_block* call (one-shot, as tracks are).  Step q (0 <= q < n_steps) falls
 * due at sample first + q * period of that block; there, register keys[k] of global instance list[i] takes
 * values[(q * n_keys + k) * count + i] - [step][key][entry], the register lists' [key][entry] per step.  Values are 32-bit
 * patterns: NaN payloads, -0 and denormals arrive as given.  Steps that fall at or beyond the block's length are dropped.
 * Afterwards a listed voice holds its last applied step, every other voice what it held.
 * DEFINITION: a block with list schedules armed leaves the caller's PCM and the handle in exactly the state that this sequence
 *   would have left: cut the block at every sample where a step falls due; in front of each piece call
 *   fxb_set_registers_list(keys, n_keys, list, count, <that step's values>) for every schedule with a step due there, in arming
 *   order.  "The state": the words on the device, fxb_save_state, what every get call returns, what the library knows about the
 *   registers.
 * Several schedules may be armed for one block, with different lists, `first` and `period`, also on the same register - two
 *   voices with note-ons at different samples - up to 64 per handle; together with fxb_set_register_track at most 16 registers
 *   have schedules.  fxb_clear_register_tracks_list drops every armed list schedule (returns 0).
 * Returns 0 - also for count == 0 or n_keys == 0, which arm nothing - or, with nothing armed and nothing changed, every shard
 *   asked before any arms, fxb_last_error naming the argument (for a list entry the caller's index): FX_E_ARG for a negative
 *   count or n_keys; null keys / list / values with something to do; n_steps < 1, period < 1 or first < 0;
 *   n_steps * n_keys * count >= 2^31; an instance outside 0..N-1 or listed twice; two keys that name one register; a 65th
 *   schedule or a 17th register with schedules; a register that has a schedule armed through fxb_set_register_track (and
 *   fxb_set_register_track refuses a register with list schedules armed); an instance that an armed list schedule already names
 *   for the same register; a register the program itself can change - the result of an instruction, the CCR, an input or an
 *   output register (named in the message): for such a register "the others keep what they have" is no value known at the head
 *   of the block.  1 for a key that is no register; FX_E_NOTREADY without a program; FX_E_MEMORY when the staging
 *   (2 * count + n_steps * n_keys * count + n_keys words per schedule, device and pinned) or the track buffer (one row of N
 *   words, padded to 256, per step and key of everything armed; below 4 GiB) could not be grown - both grow in this call,
 *   never inside a block.
 * Ordering: the call waits on the host only for the expansion of the previous block's schedules (two small kernels at the head
 *   of that block), not for the block.  The caller's arrays are free on return.  The block reads the registers' values at its
 *   own head: a fxb_set_registers_list queued between the arming and the block shows in what the other voices hold.
 * Code: as with fxb_set_register_track, the first schedule of a register makes it trackable, which asks for other code once; a
 *   real-time host arms once before fxb_prepare.  Arming a list schedule for a register that is trackable never translates
 *   again, and FXB_INFO_XLATE_CODE_HASH equals that with dense per-instance tracks on the same registers.
 * Sharded handles: every shard takes its entries with their columns of every step; on a shard without entries the registers
 *   become trackable all the same (one code for all shards) and nothing is staged or launched.
 * FXB_INFO_TRACK_LIST_EXPANDS counts the blocks that launched the expansion (fx_track_hold, fx_track_scatter). */
int fxb_set_register_tracks_list(fxb_handle* h, const char* const* keys, int n_keys, const int64_t* list, int64_t count,
                                 const float* values, int n_steps, int first, int period);
int fxb_clear_register_tracks_list(fxb_handle* h);
/* Delay-line windows by list: a window of ONE delay line of the instances a host names, written or read on the GPU - the burst
 * that excites a string or comb voice at note-on, the zeros that cut a reverb tail without touching the filter registers, an
 * impulse response or loop to pre-fill, a look at what a loop holds now.  fxb_get_tram_i handles one instance per call behind a
 * host wait and there is no setter; the save / edit / load round trip of records moves every word of every record both ways.
 *
 * which: 0 = iTRAM, 1 = xTRAM, as in fxb_get_tram_i.  values[i * n_words + j] is word first + j of global instance list[i] - one
 * voice's window is contiguous; with FXB_TRAM_BROADCAST (set only) `values` is ONE window, values[j], written to every listed
 * instance.  Words are 32-bit patterns: nothing is checked for finiteness, signalling NaNs and payloads survive.
 * What "word k" is depends on the flags.  A = the allocated slots of the line (FXB_INFO_ITRAM_SLOTS / _XTRAM_SLOTS), Z = its size.
 *   without FXB_TRAM_LOGICAL: word k is slot k - the words fxb_get_tram_i shows and a record holds at stateRows (+ iSlots) + k.
 *     Any line, ring or not; 0 <= first, 0 <= n_words, first + n_words <= A.
 *   FXB_TRAM_LOGICAL: word a is the word that a delay write at position 0 stored a + 1 writes ago (a = 0: the newest).  Only a
 *     line that is a ring (FXB_INFO_INSTANCE_RINGS bit `which`: A == Z); 0 <= first < Z, 1 <= n_words <= Z; the window may wrap
 *     the end of the ring.  With p the instance's write position word of that line (fxb_get_cursors_i [2 * which]) it is slot
 *     (p - 1 - a) mod Z, and under FX_OPT_TRAM_DANE slot (p + 1 + a) mod Z.  p is read on the device, per instance, by the kernel
 *     that moves the window: behind every queued block, whatever position each voice stands at.
 * fxb_set_tram_list: STREAM-ORDERED, in the frame of fxb_set_registers_list: it runs behind every block queued on the handle so
 *   far, on whichever stream, and in front of every block queued later; fxb_sync and every call that waits for the queued blocks
 *   cover it.  It returns when the words are staged: the caller's arrays are free on return.  A second list or instance call
 *   behind the same running block waits on the host for the first one (the staging is reused).  The program is lowered first, so
 *   that the delay memory exists.  Nothing but the words changes: no code is generated again, registers, meters, tracks and the
 *   counters are as they were.
 * fxb_get_tram_list: synchronous (it waits for everything queued).  Without FXB_TRAM_LOGICAL it equals fxb_get_tram_i word for
 *   word on every listed instance.  Repeated instances are allowed.
 * Size: the windows are staged in a block of the library's own of at most 64 MiB (device, and as much pinned), grown on demand
 *   in the call.  A call whose windows exceed it runs in pieces along the list; a SET of several pieces blocks on the host between
 *   them.  The calls are made for tens to thousands of voices times a few thousand words.
 * Returns 0 - also for count == 0, or n_words == 0 without FXB_TRAM_LOGICAL, once the other arguments have been checked (the
 *   entries of a list that is given included: n_words == 0 with an instance outside 0..N-1, or one listed twice in a set, is
 *   FX_E_ARG; a null list or null values are fine when no word moves) - or, with
 *   nothing launched and nothing changed on any shard: FX_E_ARG (fxb_last_error names the argument, and for a list entry the
 *   caller's index) for a null list or values with something to do, a negative count, count >= 2^31, `which` outside 0..1, an
 *   unknown flag bit, FXB_TRAM_BROADCAST on a get, an instance outside 0..N-1, an instance listed twice in a set (two lanes
 *   would race), a window outside the bounds above, FXB_TRAM_LOGICAL on a line that is no ring or that the program does not
 *   have; FX_E_NOTREADY without a program; FX_E_MEMORY when the staging could not be allocated, on any shard.
 * Sharded handles: every shard is asked (window, staging) before any shard changes a word; then every shard gets the entries
 *   that fall to it with their windows of `values`.  A shard without an entry launches nothing.
 * FXB_INFO_TRAM_LIST_SETS / _GETS count the launches of the two kernels (fx_tram_scatter, fx_tram_gather). */
#define FXB_TRAM_LOGICAL   (1u << 0)   /* index = age in the ring, resolved per instance on the device */
#define FXB_TRAM_BROADCAST (1u << 1)   /* set only: `values` is ONE window, written to every listed instance */
int fxb_set_tram_list(fxb_handle* h, int which, const int64_t* list, int64_t count, int first, int n_words, const float* values, unsigned flags);
int fxb_get_tram_list(fxb_handle* h, int which, const int64_t* list, int64_t count, int first, int n_words, float* values, unsigned flags);
/* one instance's delay memory as the reference holds it (which: 0 = smallDelayBuffer / iTRAM, 1 = largeDelayBuffer / xTRAM; the first
 * n_slots words; words the program cannot reach read 0) and its positions {iTRAM write, iTRAM read, xTRAM write, xTRAM read}
 * (reference smallDelayWritePos ... largeDelayReadPos, include/FX8010.h:214-217) */
int fxb_get_tram_i(fxb_handle* h, int which, int64_t instance, float* out, int n_slots);
int fxb_get_cursors_i(fxb_handle* h, int64_t instance, int32_t* out4);
/* S sample periods for all N instances.  Host buffers: synchronous (returns with `out` filled).  Caller buffers in PINNED host
 * memory (fxb_host_alloc below, hipHostMalloc / hipHostRegister, a torch pinned tensor) are processed IN PLACE: the kernel reads
 * and writes them over PCIe, no staging copies, one launch - what a real-time host wants (32-sample blocks of the 512-instruction
 * reverb: 163 840 instances inside 666.667 us; tools/realtime_capacity.py).  Pageable buffers: blocks of a few KB go through
 * pinned memory of the library, blocks of >= 32 MB are copied in, processed and copied out in overlapping pieces, everything else
 * is H2D, kernel, D2H in sequence.  `in` and `out` may be the same buffer; buffers that overlap in any other way, and buffers only
 * part of which is pinned, take the staged copies (the whole input is read before the first output is written; a buffer that
 * straddles the end of a hipHostRegister range is refused by the runtime's copy itself: FX_E_NODEVICE with its message;
 * the handle stays usable). */
int fxb_process_block(fxb_handle* h, const float* in, float* out, int n_samples);
/* in/out: [n_samples][num_channels][pitch] floats; the handle's instances are columns 0..N-1 from in/out (pass base + first
 * column).  pitch >= N (N = all instances of a sharded handle); pitch == N is fxb_process_block.  Pinned buffers: in place,
 * every shard on its own columns; columns outside the handle's range are never read or written.  Several handles may work on
 * disjoint column ranges of one buffer at the same time.  num_channels * pitch * 4 must stay below 2^32 (FX_E_ARG otherwise). */
int fxb_process_block_pitched(fxb_handle* h, const float* in, float* out, int n_samples, int64_t pitch);
/* Pinned, device-visible host memory for PCM buffers - for hosts that do not link the HIP runtime themselves (the reference's
 * callers keep their audio in plain vectors: include/FX8010.h:57; such a buffer is what to copy it into once per block).
 * NULL when the allocation fails (fx_last_create_error says why).  Free with fxb_host_free; both are thread-safe. */
void* fxb_host_alloc(int64_t bytes);
void fxb_host_free(void* p);
/* Same with device-resident buffers (hipMalloc'ed, on h's device); asynchronous on `stream`
 * (a hipStream_t, NULL = the handle's own stream).  Pair with fxb_sync(). */
int fxb_process_block_dev(fxb_handle* h, const float* d_in, float* d_out, int n_samples, void* stream);
/* single-shard handles; d_in/d_out must be device memory of h's device or device-visible host memory: anything else is
 * FX_E_ARG without a launch (the last validated buffer pair is remembered, so a real-time caller pays once).  Layout as
 * fxb_process_block_pitched; in == out or footprints that share no element.  Asynchronous like fxb_process_block_dev. */
int fxb_process_block_dev_pitched(fxb_handle* h, const float* d_in, float* d_out, int n_samples, int64_t pitch, void* stream);
/* Sharded batches: d_in[k] / d_out[k] are shard k's buffers on shard k's device, [n_samples][num_channels][n_instances of
 * the shard]; launched concurrently from the shards' own threads on their own streams.  Pair with fxb_sync(). */
int fxb_process_block_dev_shards(fxb_handle* h, const float* const* d_in, float* const* d_out, int n_samples);
/* Group buses: a shared input and / or a mixed output per group of `group` consecutive instances.  G = fxb_bus_groups(h, group) =
 * ceil(N / group); group g holds instances g*group .. min((g+1)*group, N) - 1 (the last one may be short; group >= N is one group).
 *   FXB_BUS_SHARED_IN  `in` is [n_samples][num_channels][G]: instance n reads column n / group (one signal through `group`
 *                      instances that differ in their controls - a parameter sweep).  Without it `in` is [..][N] as ever.
 *   FXB_BUS_MIX_OUT    `out` is [n_samples][num_channels][G]: column g is the sum of the group's outputs (voices onto a bus), in
 *                      fp32, round to nearest, never fused, denormals kept, in exactly this order: 64 partial sums p[0..63] start
 *                      at +0.0f; for j = 0, 1, ... every member m = j*64 + l of the group that exists is added to p[l]; then for
 *                      step = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l + step] for l < step; the sum is p[0].  Without it `out` is
 *                      [..][N].
 * flags == 0 is fxb_process_block.  The instances' state afterwards is what fxb_process_block on the expanded input leaves; control
 * tracks armed for the block apply.  Only the [..][G] sides cross PCIe: a small kernel expands the input into a per-instance block
 * in device memory, the program runs on it in place, a second kernel adds the groups up.
 * Host entry: synchronous; pinned buffers (fxb_host_alloc ...) are read and written in place by those kernels, others are staged.
 * Device entry: single-shard handles, buffers checked like fxb_process_block_dev_pitched's, asynchronous on `stream`.
 * Sharded handles: every shard must begin at a multiple of `group` (fxb_shard_plan), else FX_E_ARG.
 * FX_E_ARG (nothing launched, nothing changed): group < 1, unknown flag bits, a null buffer with n_samples > 0, `in` and `out`
 * overlapping without being the same buffer with the same layout, num_channels * row length * 4 >= 2^32 in any layout. */
#define FXB_BUS_SHARED_IN (1u << 0)
#define FXB_BUS_MIX_OUT   (1u << 1)
int64_t fxb_bus_groups(fxb_handle* h, int64_t group);   /* G, or FX_E_ARG */
int fxb_process_block_bus(fxb_handle* h, const float* in, float* out, int n_samples, int64_t group, unsigned flags);
int fxb_process_block_bus_dev(fxb_handle* h, const float* d_in, float* d_out, int n_samples, int64_t group, unsigned flags, void* stream);
/* Bus gains: a weight per (channel, instance) on the way into the sum of FXB_BUS_MIX_OUT - a level per voice, a pan over the
 * channels of the bus, a mute - with a ramp over one block.  Gains are a mode of the handle like the meters, off by default: no
 * flag bit of the block calls is taken, and while they are off the mix is the unweighted sum above, by the same kernel as ever.
 *
 * The definition.  The handle holds two sets per (channel c, instance n): the CURRENT gains a and the TARGET b.  While gains are
 * off, a counts as 1.0f everywhere.
 *   fxb_bus_set_gains(h, gains, 0)   a = b = gains.
 *   fxb_bus_set_gains(h, gains, 1)   b = gains, a stays: a ramp is now PENDING.
 *   A second call before a mixing block replaces b; with ramp = 0 it also cancels the pending ramp.
 *   The next block with FXB_BUS_MIX_OUT consumes a pending ramp: afterwards a = b.  A block without FXB_BUS_MIX_OUT ignores the
 *   gains and leaves a pending ramp pending.
 * For one call of S samples (S is the caller's n_samples, never that of a piece the runtime cuts the block into), the member of
 * channel c and instance n at sample s (0-based) has the output word y and the weight w, everything in fp32, round to nearest,
 * never fused, denormals kept:
 *   no ramp pending:  w = b
 *   ramp pending:     w = b                      if s == S - 1
 *                     w = a + (b - a) * t        otherwise, with t = (float)(s + 1) * r and r = 1.0f / (float)S - (b - a), the
 *                                                product and the sum are three roundings, r is one fp32 division
 *   term = (w == 0.0f) ? +0.0f : w * y           either sign of zero: a muted member contributes +0.0f whatever y is, NaN and Inf
 *                                                included
 * The terms then go through exactly the order of the unweighted sum: 64 partial sums start at +0.0f, member m = j*64 + l, where it
 * exists, is added to p[l] for j ascending, the step = 32 ... 1 tree follows; members that do not exist are not added.
 * Consequences:
 *   Gains of 1.0f everywhere give the words of the unweighted sum.  NaNs stay NaNs; their payload is not promised.
 *   A ramp is per call: two calls of 16 + 17 samples are not one of 33 while a ramp is pending.  Without one they are.
 *   The last sample of a ramp block carries exactly b.
 *   The meters read the per-instance block in front of the mix and are therefore pre-fader: a muted NaN voice still counts in
 *   `nonfinite`.  That is the intended pairing: fxb_meter_read tells which instance to mute.
 *
 * fxb_bus_set_gains: gains is [num_channels][N] by global instance, or NULL = gains off.  ramp is 0 or 1.  Every value must be
 *   finite, else FX_E_ARG and nothing changes (a bad ramp likewise).  The array is copied through pinned memory of the library and
 *   is the caller's again on return.  Works before a program is loaded; the gains survive program loads; they are not part of the
 *   state image or of instance records, and fxb_copy_instances / fxb_reset_instances do not touch them: a gain belongs to the mixer
 *   slot, not to the voice.  All allocation (two blocks of num_channels * N floats per shard, the staging) happens in this call,
 *   never inside a block; FX_E_MEMORY leaves the gains as they were on every shard.  NULL waits for the queued blocks and frees;
 *   if that wait reports a device error, the code is returned and the shard it happened on keeps its gains and their memory (on a
 *   handle of several shards the others have switched theirs off: after a device error call NULL again or destroy the handle).
 * Ordering: a block queued on whatever stream keeps the gains it was queued with - a set after it does not disturb it - and a
 *   later block on whatever stream sees the new gains; fxb_sync covers all of it.  (A set does not wait for the queued block on the
 *   host; a second set behind the same running block does.)
 * fxb_bus_get_gains: [num_channels][N], the gains in force - a; after a ramp has been consumed that is its target.  Waits as
 *   fxb_sync does.  FX_E_ARG while gains are off.
 * FXB_INFO_BUS_GAIN_BLOCKS counts the bus blocks mixed with gains. */
int fxb_bus_set_gains(fxb_handle* h, const float* gains, int ramp);
int fxb_bus_get_gains(fxb_handle* h, float* gains);
/* Gain sets by list: the faders that moved, and only those.  A mixer moves a few faders per block; the full sets above send every
 * gain again - 4 * num_channels * N bytes over PCIe for the bus gains, and a wait for every queued block for the send and feed
 * gains.  These three calls write the listed weights of the structure in force and leave all others alone: the list and the values
 * go through pinned memory of the library (the arrays are the caller's again on return) and a small kernel scatters them on the
 * device.  Nothing else changes: not what a block does with a, b and a pending ramp (w, t, r, the w == 0 mute, the summation
 * orders, which block consumes the ramp), not what fxb_bus_get_gains / _sends / _feeds return (a, for listed and unlisted indices).
 *
 * The definition, in the terms of "Bus gains".  The structure - the bus gains, the weights of the sends, the weights of the feeds -
 * holds a, b and the handle-wide flag PENDING.  `gains` is [num_channels][count] with a row pitch of exactly count; column k
 * belongs to list[k] - a global instance number in 0..N-1 for the bus gains, a global entry index in 0..E-1 for the sends and the
 * feeds (the index into the `members` / `sources` array the structure was set with, which is what fxb_bus_get_sends / _feeds
 * return).  L is the set of listed indices.
 *   ramp = 1, none pending   a := b everywhere (what "a counts as the old b" already means); b[i] := gains[k] for i in L; a ramp
 *                            is now pending.
 *   ramp = 1, one pending    b[i] := gains[k] for i in L; a stays everywhere.
 *   ramp = 0                 a[i] := b[i] := gains[k] for i in L, and nothing else.  A pending ramp STAYS PENDING for the indices
 *                            outside L; a listed index has a = b and so carries a constant weight through the ramp block.  This is
 *                            the one place where a list set is not a full set restricted to L: a full set with ramp = 0 cancels
 *                            the ramp.
 *   Indices outside L keep their a and their b in every case.
 * Feeds that are unweighted: the call makes them weighted first, with a = b = 1.0f everywhere (the rule of fxb_bus_set_feed_gains),
 *   then applies the above; from then on the entries of an instance with F = 1 go through the multiply - the move of bit patterns
 *   belongs to unweighted feeds only.
 * count == 0 returns 0 and changes nothing (unweighted feeds stay unweighted).
 * FX_E_ARG, with nothing launched and nothing changed: ramp not 0 or 1, count < 0, a null list or null gains with count > 0, an
 *   index outside its range, a REPEATED index (two lanes would race for one word), a value that is not finite, and the mode being
 *   off - bus gains off, sends off, feeds off: a list call does not switch a mode on, the full set does that.
 * FX_E_MEMORY leaves everything as it was on every shard.  The staging - count * (num_channels + 1) words in device memory and as
 *   many pinned - is grown on demand in the call, never inside a block, and freed with the handle.
 * Ordering: that of fxb_bus_set_gains, for all three.  The call does not wait on the host for queued blocks; a block queued on
 *   whatever stream keeps the weights it was queued with, a later block on whatever stream sees the new ones, fxb_sync covers all
 *   of it.  A second list set behind the same running block does wait on the host for the first one's copy (the staging is
 *   reused), as a second full gain set does.  The full fxb_bus_set_send_gains / _feed_gains keep their wait for everything queued,
 *   which includes a list set still in flight.
 * Sharded handles: every shard gets the entries that fall to it; a shard without one launches nothing and still follows the
 *   handle-wide "none pending -> pending" step, so that fxb_bus_get_gains and the next ramp block see one state on all shards.
 * FXB_INFO_GAIN_LIST_SETS counts the launches of the scatter kernel (fx_gain_scatter). */
int fxb_bus_set_gains_list(fxb_handle* h, const int64_t* list, int64_t count, const float* gains, int ramp);
int fxb_bus_set_send_gains_list(fxb_handle* h, const int64_t* entries, int64_t count, const float* gains, int ramp);
int fxb_bus_set_feed_gains_list(fxb_handle* h, const int64_t* entries, int64_t count, const float* gains, int ramp);
/* Bus taps: per-instance monitor outputs by list beside the mixed bus - solo, PFL, a recording of one voice, a look at the voice
 * whose meter went non-finite - without taking all N columns over PCIe.  Taps are a mode of the handle like the meters and the
 * gains, off by default: no flag bit is taken and no existing signature or behaviour changes.
 *
 * fxb_bus_set_taps: list holds T = count global instance numbers in 0..N-1, in any order; repeats are allowed (one voice may feed
 *   two monitor columns).  count == 0 (any list) turns taps off and frees their memory.  FX_E_ARG with nothing changed: count < 0,
 *   count > 65 536 (a tap set is a monitor selection, not a second output path: the cap keeps the device list and every row of
 *   tap_out small), a null list with count > 0, an entry outside 0..N-1.  The list is copied before the call returns.  All
 *   allocation for the list happens here, on every shard before any shard's list changes: FX_E_MEMORY leaves the old taps in force
 *   everywhere.  The call waits for the queued blocks as fxb_meter_enable does, so a queued block keeps the taps it was queued
 *   with.  Works before a program is loaded; the taps survive program loads; they are not part of the state image or of instance
 *   records, and fxb_copy_instances / fxb_reset_instances do not touch them: a tap belongs to the mixer slot, not to the voice.
 * fxb_bus_get_taps: returns T (0 while taps are off) and copies min(T, cap) entries; list may be NULL with cap 0.
 *
 * The tapped block.  tap_out is [n_samples][num_channels][T] with a row pitch of exactly T: tap_out[(s*C + c)*T + t] is the 32-bit
 * word that fxb_process_block on the expanded input writes at out[(s*C + c)*N + list[t]], moved as a bit pattern (NaN payloads
 * survive).  Taps are pre-fader and pre-mute like the meters: a voice whose gain is 0 is still heard on its tap, which is what PFL
 * means.  `out` (the mix), instance state, meters, gains with their pending ramp, armed control tracks and every other FXB_INFO_*
 * counter are exactly what fxb_process_block_bus with the same arguments leaves.  A block cut into sample ranges by the 64 MiB
 * scratch delivers each range's rows to tap_out + first_row * T.  tap_out == NULL is fxb_process_block_bus / _bus_dev.
 * n_samples == 0 lowers the program and returns 0.  One small kernel per range gathers the columns from the per-instance block in
 * device memory, between the program and the mix.
 * FX_E_ARG (nothing launched, nothing changed): tap_out non-null while taps are off; tap_out non-null without FXB_BUS_MIX_OUT in
 * flags (without it `out` already holds every column); tap_out sharing a byte with the footprint of `in` or of `out`; every
 * refusal of fxb_process_block_bus*; the device entry on a handle of several shards or with a d_tap_out the device cannot address
 * over the whole block (checked and remembered like the other two buffers).
 * Host entry: synchronous.  A pinned tap_out (fxb_host_alloc ...) is stored to in place over PCIe; any other goes through a device
 * staging block that grows on demand and is copied out before the call returns (FX_E_MEMORY: nothing launched).  in / out keep
 * their own in-place / staged decision.  Device entry: asynchronous on `stream`, covered by fxb_sync.
 * Sharded handles: each shard gets the entries of the list that fall into its range and writes only their columns of the caller's
 * full-width tap_out; a shard with no entry launches no tap kernel.  The group-alignment condition of bus blocks applies.
 * FXB_INFO_BUS_TAP_BLOCKS counts the bus blocks that were given a tap_out: once per block and shard, like FXB_INFO_BUS_GAIN_BLOCKS. */
int     fxb_bus_set_taps(fxb_handle* h, const int64_t* list, int64_t count);
int64_t fxb_bus_get_taps(fxb_handle* h, int64_t* list, int64_t cap);
int     fxb_process_block_bus_tap(fxb_handle* h, const float* in, float* out, float* tap_out, int n_samples, int64_t group, unsigned flags);
int     fxb_process_block_bus_tap_dev(fxb_handle* h, const float* d_in, float* d_out, float* d_tap_out, int n_samples, int64_t group, unsigned flags,
                                      void* stream);
/* Bus sends: aux buses by member list beside the group mix - an effects bus fed by "a little of every voice", a bus whose members
 * are not K consecutive slots, a voice on several buses at once - without taking all N columns over PCIe.  Sends are a mode of
 * the handle like the meters, the gains and the taps, off by default: no flag bit is taken and no existing signature or result
 * changes.
 *
 * The structure.  There are A = n_aux aux buses.  Bus b owns the entries e = offsets[b] .. offsets[b+1] - 1 of `members` (CSR:
 * offsets has A + 1 values, offsets[0] = 0, non-decreasing, E = offsets[A]); members[e] is a global instance number.  Any order
 * and repeats are allowed, within a bus and across buses; an empty bus is allowed.  gains is [num_channels][E], one weight per
 * channel and entry; NULL means 1.0f everywhere.
 *
 * fxb_bus_set_sends: n_aux == 0 turns sends off and frees their memory.  FX_E_ARG with nothing changed: A < 0 or A > 65 536,
 *   E > 16 777 216, a null array that is needed, offsets not as above, a member outside 0..N-1, a non-finite gain.  The arrays are
 *   copied before the call returns.  All allocation happens here, on every shard before any shard changes: FX_E_MEMORY leaves the
 *   old sends in force everywhere.  The call waits for the queued blocks as fxb_bus_set_taps does.  It sets a = b = gains and
 *   cancels a pending ramp.  Works before a program is loaded; the sends survive program loads; they are not part of the state
 *   image or of instance records, and fxb_copy_instances / fxb_reset_instances do not touch them.
 * fxb_bus_set_send_gains: replaces the weights of the structure in force ([num_channels][E], finite, else FX_E_ARG; FX_E_ARG
 *   while sends are off) by the current / target state machine of fxb_bus_set_gains: ramp = 0: a = b = gains; ramp = 1: b = gains
 *   and a ramp is pending (a is the old b, or stays where a ramp was pending already).  The next block that is given an aux_out
 *   consumes the ramp; blocks without one leave it pending.  Queued blocks keep the weights they were queued with (the call waits
 *   for them).
 * fxb_bus_get_sends: returns E (0 while sends are off), stores A to *n_aux, and copies what fits: offsets[0 .. min(A + 1,
 *   off_cap) - 1], and the entries below cap of members and of every channel row of gains (row pitch E).  gains is a, as
 *   fxb_bus_get_gains returns.  Any pointer may be NULL.
 *
 * The block.  aux_out is [n_samples][num_channels][A] with a row pitch of exactly A.  aux_out == NULL is
 * fxb_process_block_bus_tap[_dev] with the remaining arguments.  With it, `out`, tap_out, instance state, meters, the bus gains
 * with their pending ramp, armed control tracks and every other FXB_INFO_* counter are exactly what that call leaves.
 * Sends are PRE-FADER: they read the same per-instance block as the meters and the taps, in front of the mix; the bus gains and
 * their mute do not act on them.  A host that wants a post-fader send multiplies when it sets the send gains; a NaN voice is kept
 * off an aux bus by a send gain of 0.
 *
 * The sum.  Let T(v_0 .. v_{L-1}) be the order of the group mix: 64 partial sums p[0..63] start at +0.0f; for j = 0, 1, ..
 * every v_{j*64+l} that exists is added to p[l]; then for step = 32 .. 1: p[l] = p[l] + p[l+step] for l < step; T is p[0].
 * Everything is fp32, round to nearest, never fused, denormals kept.  For bus b, channel c and sample s of a call of S samples,
 * the entry at position m (e = offsets[b] + m) has the term (w == 0.0f) ? +0.0f : w * y, where y is the word fxb_process_block on
 * the expanded input writes at out[(s*C + c)*N + members[e]] and w comes from that entry's a / b and the ramp exactly as the
 * "Bus gains" comment defines it (t = (float)(s+1) * r, r = 1.0f / (float)S with S the caller's block, exactly b on the last
 * sample).  The positions are cut into chunks of 1 024: c_q = T(the terms of positions q*1024 .. q*1024 + 1023 that exist).
 * With M_b <= 1 024 entries the bus word is c_0 itself (+0.0f for M_b = 0); otherwise it is T(c_0 .. c_{Q-1}), Q = ceil(M_b /
 * 1024).  So a bus of at most 1 024 entries that lists the members of a group in ascending order with that group's gains carries
 * the words of the (weighted) group mix; a larger one does not - the price of many wavefronts per bus.  NaN payloads are not
 * promised.  1 024 is part of the contract.
 *
 * FX_E_ARG (nothing launched, nothing changed): aux_out non-null while sends are off; aux_out non-null without FXB_BUS_MIX_OUT
 * (the same reason as for taps); aux_out sharing a byte with the footprint of `in`, `out` or tap_out; every refusal of
 * fxb_process_block_bus_tap*; the device entry on a handle of several shards or with a d_aux_out the device cannot address over
 * the whole block (checked and remembered like the other buffers).
 * Routes are those of the tap rows, independently of how in / out / tap_out go: a pinned aux_out is stored to in place; any
 * other goes through a device staging block that grows on demand in front of the block's first launch (FX_E_MEMORY: nothing
 * launched) and is copied out before the call returns.  A block cut into sample ranges by the 64 MiB scratch delivers each
 * range's rows to aux_out + first_row * A.  n_samples == 0 lowers the program and returns 0.
 * Sharded handles: there is no collective on the data path, and a sum across shards would make the bits depend on the split, so
 * fxb_bus_set_sends is FX_E_ARG when the members of one aux bus fall into more than one shard (the message names the bus;
 * fxb_shard_plan tells the boundaries).  Otherwise each shard gets its buses and writes only their columns of the caller's
 * full-width aux_out; a shard with no bus launches nothing.
 * FXB_INFO_BUS_SEND_BLOCKS counts the bus blocks that were given an aux_out: once per block and shard. */
int     fxb_bus_set_sends(fxb_handle* h, int64_t n_aux, const int64_t* offsets, const int64_t* members, const float* gains);
int     fxb_bus_set_send_gains(fxb_handle* h, const float* gains, int ramp);
int64_t fxb_bus_get_sends(fxb_handle* h, int64_t* n_aux, int64_t* offsets, int64_t off_cap, int64_t* members, float* gains, int64_t cap); /* returns E */
int     fxb_process_block_bus_aux(fxb_handle* h, const float* in, float* out, float* tap_out, float* aux_out, int n_samples, int64_t group, unsigned flags);
int     fxb_process_block_bus_aux_dev(fxb_handle* h, const float* d_in, float* d_out, float* d_tap_out, float* d_aux_out, int n_samples, int64_t group, unsigned flags,
                                      void* stream);
/* Bus feeds: per-instance input by source list, summed on the device - the sends mirrored on the input side.  Every instance owns
 * a list of columns of a narrow source block [n_samples][num_channels][M], each with a weight per channel; a kernel builds the
 * per-instance [..][N] block from the lists where FXB_BUS_SHARED_IN builds it from n / group.  With them the aux rows of one
 * handle feed the effect instances of a second one without leaving the device, a sweep may have members that are not `group`
 * neighbours, a voice may hear a mix of two sources (a side-chain, a mix-minus), and an input fades in over one block.  Feeds
 * are a mode of the handle like the meters, the gains, the taps and the sends, off by default: no flag bit is taken and no
 * existing signature or result changes.
 *
 * The structure.  There are M = n_src source columns.  Instance n (a global instance number) owns the entries e = offsets[n] ..
 * offsets[n+1] - 1 of `sources` (CSR by instance: offsets has N + 1 values, offsets[0] = 0, non-decreasing, E = offsets[N] <=
 * 16 777 216); sources[e] is a column in 0..M-1.  Any order and repeats are allowed, within a list and across lists; an instance
 * may have no entry.  gains is [num_channels][E], one weight per channel and entry; NULL means UNWEIGHTED, which is not the same
 * as 1.0f everywhere (below).
 *
 * fxb_bus_set_feeds: n_src == 0 turns feeds off and frees their memory.  FX_E_ARG with nothing changed: M < 0,
 *   num_channels * M * 4 >= 2^32, E > 16 777 216, a null array that is needed, offsets not as above, a source outside 0..M-1, a
 *   non-finite gain.  The arrays are copied before the call returns.  All allocation happens here, on every shard before any
 *   shard changes: FX_E_MEMORY leaves the old feeds in force everywhere.  The call waits for the queued blocks as fxb_bus_set_taps
 *   does.  It sets a = b = gains and cancels a pending ramp.  Works before a program is loaded; the feeds survive program loads;
 *   they are not part of the state image or of instance records, and fxb_copy_instances / fxb_reset_instances do not touch them.
 * fxb_bus_set_feed_gains: replaces the weights of the structure in force ([num_channels][E], finite, else FX_E_ARG; FX_E_ARG
 *   while feeds are off) by the current / target state machine of fxb_bus_set_gains: ramp = 0: a = b = gains; ramp = 1: b = gains
 *   and a ramp is pending (a is the old b, or stays where a ramp was pending already; out of unweighted, a is 1.0f everywhere).
 *   NULL returns to unweighted and drops a pending ramp.  The next FEED block consumes a pending ramp; other blocks leave it
 *   pending.  Queued blocks keep the weights they were queued with (the call waits for them).
 * fxb_bus_get_feeds: returns E (0 while feeds are off), stores M to *n_src, and copies what fits: offsets[0 .. min(N + 1,
 *   off_cap) - 1], and the entries below cap of sources and of every channel row of gains (row pitch E).  gains is a, as
 *   fxb_bus_get_gains returns; 1.0f everywhere while the feeds are unweighted.  Any pointer may be NULL.
 *
 * The block.  src is [n_samples][num_channels][M] with a row pitch of exactly M; it replaces `in`.  flags may carry
 * FXB_BUS_MIX_OUT only.  group, out, tap_out and aux_out mean what they mean to fxb_process_block_bus_aux[_dev], and so do its
 * refusals, routes, pieces and event ordering.  n_samples == 0 lowers the program and returns 0.
 *
 * The definition.  Everything is fp32, round to nearest, never fused, denormals kept.  For instance n, channel c and sample s of
 * a call of S samples, the entries are k = 0..F-1 (e = offsets[n] + k) and x_k is the word src[(s*C + c)*M + sources[e]].
 *   F = 0            the input word is +0.0f.
 *   unweighted       term_k = x_k.  With F = 1 the word is MOVED AS A 32-BIT PATTERN: a NaN keeps its payload, -0 stays -0.
 *   weighted         term_k = (w == 0.0f) ? +0.0f : w * x_k, where w comes from that entry's a / b and the ramp exactly as the
 *                    "Bus gains" comment defines it (t = (float)(s+1) * r, r = 1.0f / (float)S with S the caller's block, never
 *                    a piece; exactly b on the last sample).
 *   the word         term_0 for F = 1, else ((term_0 + term_1) + term_2) + ... in entry order: it starts from term_0, not from
 *                    zero.
 * NaN payloads are not promised once an addition or a multiplication has happened.  As numpy, over float32 arrays:
 *   word = zeros(N); for k in range(max F): has = k < F; e = offsets[:-1] + k
 *       term = x[sources[e]] if unweighted else where(w[e] == 0, +0.0, w[e] * x[sources[e]])
 *       word = where(has, term if k == 0 else word + term, word)
 * The instances' state, `out`, meters, taps, sends, bus gains and armed control tracks afterwards are exactly what
 * fxb_process_block_bus_aux leaves on the [S][C][N] input this defines.
 * A consequence: unweighted feeds with M = G, one entry per instance and sources[n] = n / K reproduce FXB_BUS_SHARED_IN with
 * group K, word for word.  A zero gain keeps a NaN source column out of an instance.
 *
 * FX_E_ARG (nothing launched, nothing changed), beyond every refusal of fxb_process_block_bus_aux*: feeds off; FXB_BUS_SHARED_IN
 * in flags; src null with n_samples > 0; src sharing a byte with `out`, tap_out or aux_out (there is no in-place form: the
 * layouts differ); the device entry on a handle of several shards or with a d_src the device cannot address.
 * Gathers hit device memory only: every word of src is read many times, so the runtime copies the caller's src rows, pinned or
 * pageable, into a device block [rows][M] that grows on demand in front of the block's first launch (FX_E_MEMORY: nothing
 * launched); only a src that the pointer attributes show to be device memory of the handle's device is gathered in place -
 * through either entry.  out / tap_out / aux_out keep their own in-place / staged decisions.
 * Sharded handles: each shard gets the lists of its own instances, reads the caller's full-width src and stages the rows on its
 * own device.  The input side has no sum across shards: no structure is refused for straddling, and shards need not begin at a
 * multiple of anything for the feed side; FXB_BUS_MIX_OUT keeps its own rule.
 * FXB_INFO_BUS_FEED_BLOCKS counts the feed blocks: once per block and shard. */
int     fxb_bus_set_feeds(fxb_handle* h, int64_t n_src, const int64_t* offsets, const int64_t* sources, const float* gains);
int     fxb_bus_set_feed_gains(fxb_handle* h, const float* gains, int ramp);
int64_t fxb_bus_get_feeds(fxb_handle* h, int64_t* n_src, int64_t* offsets, int64_t off_cap, int64_t* sources, float* gains, int64_t cap); /* returns E */
int     fxb_process_block_bus_feed(fxb_handle* h, const float* src, float* out, float* tap_out, float* aux_out, int n_samples, int64_t group, unsigned flags);
int     fxb_process_block_bus_feed_dev(fxb_handle* h, const float* d_src, float* d_out, float* d_tap_out, float* d_aux_out, int n_samples, int64_t group, unsigned flags,
                                       void* stream);
/* Instance-major blocks: one interleaved stream per instance, transposed on the device.  Instance n's input is the
 * n_samples * num_channels floats at in + n * in_stride, ordered [sample][channel] - what n_samples calls of the reference's
 * process() consume and what a WAV file holds - and its output goes to out + n * out_stride the same way.
 *   Strides are in floats.  0 means packed (n_samples * num_channels).  A stride above the run is the useful case: a host that
 *   holds a whole file or a ring per instance passes base + f0 * num_channels with the stride of the whole allocation and walks
 *   through it block by block without copying.  The words between two runs are never read and never written.
 *   Nothing beyond 4-byte alignment is assumed of a base or a stride.  n * stride * 4 may exceed 2^32 (the offset of an instance
 *   is 64-bit arithmetic); n_samples * num_channels must stay below 2^31.
 * Results and instance state afterwards are exactly those of fxb_process_block on the transposed input: two small kernels
 * surround the unchanged launch of the program - a gather from the streams into a per-instance [sample][channel][N] block in
 * device memory (the scratch block of bus blocks), the program in place on it, a scatter back to the streams.  Every word is moved
 * as a 32-bit pattern.  Control tracks armed for the block apply; n_samples == 0 lowers the program and returns 0.  Blocks whose
 * scratch would exceed 64 MiB run in consecutive sample ranges (with a track armed the block stays whole).  Bus blocks and
 * instance-major blocks may alternate on one handle, on different streams.  FXB_INFO_IMAJOR_BLOCKS counts these blocks,
 * FXB_INFO_BUS_BLOCKS does not.
 * Overlap: in == out with in_stride == out_stride is allowed (a range of samples is wholly gathered before anything of it is
 * scattered); so are footprints - N runs of n_samples * num_channels floats at the stride - that share no element.  Any other
 * overlap is FX_E_ARG.
 * Host entry: synchronous.  Pinned buffers (fxb_host_alloc ...) are read and written in place by the two kernels, no copies
 * (FXB_INFO_HOST_INPLACE_BLOCKS); other memory is staged with 2-D copies of the N runs and transposed from the staging block
 * (FXB_INFO_HOST_STAGED_BLOCKS).
 * Device entry: single-shard handles, buffers checked like fxb_process_block_bus_dev's and remembered, asynchronous on `stream`,
 * covered by fxb_sync.
 * Sharded handles: shard k works on the runs from in + first_k * in_stride on, on its own thread and stream; in place where its
 * device can address the buffer, staged (that shard only) otherwise.  No condition on the shard boundaries.
 * FX_E_ARG (nothing launched, nothing changed): n_samples < 0, a negative stride or one above 0 and below
 * n_samples * num_channels, a null buffer with n_samples > 0, overlap as above, the device entry on a handle of several shards or
 * with memory the device cannot address. */
int fxb_process_block_imajor(fxb_handle* h, const float* in, float* out, int n_samples, int64_t in_stride, int64_t out_stride);
int fxb_process_block_imajor_dev(fxb_handle* h, const float* d_in, float* d_out, int n_samples, int64_t in_stride, int64_t out_stride, void* stream);
/* Output meters: per instance and channel the peak, the energy, how often the output sat at the FX8010's +-1 saturation rail and
 * how many of its samples were non-finite - computed on the device, accumulated there across blocks, read when the host wants
 * them.  Metering is a mode of the handle, off by default; with it off nothing below costs anything.
 *
 * The definition.  Each pair (channel c, instance n) has four accumulators.  After reset they are energy = +0.0 (fp64),
 * peak = +0.0f, full_scale = 0 and nonfinite = 0 (both uint32).  For every output word y of that column, in sample order:
 *   fin = |y| < +Inf.  This is false for NaN and +-Inf.
 *   w = fin ? |y| : +0.0f.
 *   energy = energy + (double)w * (double)w.  The product of two fp32 values is exact in fp64.  There is therefore one rounding
 *     per sample, in the add, and fused or unfused arithmetic gives the same bits.
 *   peak = max(peak, w).
 *   full_scale += (fin && |y| >= 1.0f).
 *   nonfinite += !fin.
 * The two counters saturate at 0xFFFFFFFF.
 * The order is sequential over the samples of a block, then over blocks in the order they were queued.  The accumulators are
 * carried in device memory between launches.  A stream cut into blocks of 16 + 17 samples therefore gives the same bits as one
 * block of 33.  The same holds for a block that the runtime cuts into pieces.  The pieces are those of the 64 MiB bus scratch and
 * those of a pageable host block of 32 MB and more; a block with a control track armed that the interpreter and HIP C++ tiers cut
 * at its change points is metered segment by segment, in order, to the same bits.
 *
 * Where the meters look.  A small kernel follows every launch of the program on the same stream and reads the per-instance
 * output block exactly where that launch wrote it:
 *   device entries            the caller's d_out, at its pitch;
 *   staged host blocks        the library's device staging buffer;
 *   pinned host blocks        processed in place: the caller's pinned memory, which the meter kernel reads BACK over PCIe (the
 *                             block crosses the link a third time: real-time hosts that want meters use bus blocks);
 *   bus blocks                the per-instance scratch block in device memory, between the program and the mix or the copy out:
 *                             the per-instance output still never leaves the device, and every instance has its figures.
 *   instance-major blocks     the same scratch block, between the program and the scatter to the streams: the meter reads
 *                             device memory, whichever memory the streams live in.
 * While metering is on, fxb_last_kernel_ms and fxb_shard_kernel_ms cover the program's launch plus its meter launch (the meter
 * is queued in front of the event that ends the measurement, so that every wait for a block also covers the meter's read of the
 * caller's buffer).
 *
 * fxb_meter_enable: on != 0 allocates and zeroes the accumulator rows on every shard (20 bytes per instance and channel), 0 frees
 *   them.  Enabling twice is a no-op that keeps the values.  FX_E_MEMORY leaves metering off and the handle usable.  All device
 *   allocation for metering happens here, never inside a block.  Waits for the blocks that have been queued.
 * fxb_meter_read: every array is [num_channels][N] by global instance; any pointer may be NULL.  Synchronous: waits as fxb_sync
 *   does, copies, and with reset != 0 zeroes the accumulators after the copy.  FX_E_ARG while metering is off.
 * fxb_meter_samples: the sample periods metered since the last reset, or FX_E_ARG while metering is off.
 * A program load (fxb_load_file / fxb_load_text) resets the meters and keeps them enabled.  Meters are not part of the state
 * image: fxb_save_state and fxb_load_state leave them alone.  FXB_INFO_METER_LAUNCHES counts the meter kernel's launches. */
int fxb_meter_enable(fxb_handle* h, int on);
int fxb_meter_read(fxb_handle* h, double* energy, float* peak, uint32_t* full_scale, uint32_t* nonfinite, int reset);
int64_t fxb_meter_samples(fxb_handle* h);
/* Meter queries by list: the meters are what the device produces for the host to act on - which voices went non-finite (mute
 * them: fxb_bus_set_gains_list), which have decayed below a level (their slots are free: fxb_reset_instances,
 * fxb_set_tram_list), what the figures of these twenty voices are.  The answer to each is a short list; fxb_meter_read moves every
 * row of every instance and can only zero every accumulator.  These calls select, read and reset by list, on the GPU.
 *
 * fxb_meter_select: the definition.  v(c, n) is accumulator `stat` (FXB_METER_ENERGY, _PEAK, _FULL_SCALE, _NONFINITE) of channel c
 *   and global instance n, taken as a real number - the conversions of a float or a uint32 to double are exact.  V(n) = max over
 *   the handle's channels of v(c, n).  No rounding occurs anywhere.  Instance n in first .. first + n_range - 1 matches when
 *   V(n) >= threshold, or, with FXB_METER_BELOW, when V(n) < threshold.  M is the number of matches.  The call writes the
 *   min(M, cap) SMALLEST matching global instance numbers to `list`, ascending, and returns M; M may exceed cap, and `list` beyond
 *   min(M, cap) is not touched.  cap == 0 is a count query.  n_range == 0 returns 0 without a launch.  The list is compacted on
 *   the device - per-wavefront counts, an exclusive scan over the chunk counts, an emit pass; no atomics decide a position - so
 *   it is the same run to run, and only min(M, cap) numbers cross PCIe.
 *   Synchronous: it waits as fxb_sync does, which covers a list reset still in flight, and it changes nothing.
 *   threshold may be +-Inf; NaN is FX_E_ARG.  Also FX_E_ARG, with nothing launched: metering off, stat outside 0..3, an unknown
 *   flag bit, first < 0, n_range < 0 or first + n_range > N, cap < 0, a null list with cap > 0.  FX_E_MEMORY when the staging -
 *   min(cap, n_range) instance numbers plus a count per chunk of 256 instances, in device memory and pinned, grown on demand in
 *   the call and freed with the handle - cannot be allocated.
 *   Sharded handles: each shard answers for the part of the range it owns; the parts are concatenated in shard order, which is
 *   ascending; cap applies to the whole result and the return value is the sum.  A shard whose part is empty launches nothing.
 * fxb_meter_read_list: every array is [num_channels][count] with a row pitch of exactly `count`; column k belongs to list[k]; any
 *   array pointer may be NULL.  The values are, bit for bit, those fxb_meter_read puts at [c][list[k]].  Synchronous.  Repeats are
 *   allowed when reset == 0.  With reset != 0 the four accumulators of every listed (channel, instance) are zero afterwards and
 *   nothing else changes; a repeated instance is then FX_E_ARG; the read and the zeroing of one column happen in one lane of one
 *   launch.  count == 0 returns 0.  FX_E_ARG otherwise as for fxb_get_registers_list: a negative count, a null list with
 *   count > 0, an instance outside 0..N-1, count >= 2^31, metering off.  FX_E_MEMORY when the staging cannot be allocated: nothing
 *   is zeroed on any shard.
 * fxb_meter_reset_list: the four accumulators of every channel of the listed instances become +0.0, +0.0f, 0, 0 - a slot reused
 *   at note-on gets a fresh meter without wiping everyone's.  Repeats are allowed.  STREAM-ORDERED, in the frame of
 *   fxb_set_registers_list: it runs on the handle's stream behind every block queued so far on whichever stream - that block's
 *   meter launch included - and in front of every block queued later; it waits on the host only for a previous list or instance
 *   call whose staging it reuses.  The caller's list is free on return.  fxb_sync, fxb_meter_read, fxb_meter_read_list and
 *   fxb_meter_select cover it.  Refusals as for fxb_meter_read_list.  Sharded handles: every shard is asked for its staging before
 *   any shard changes a word; a shard without an entry launches nothing.
 * fxb_meter_samples stays the handle-wide count of sample periods since the last FULL reset (fxb_meter_read with reset, a program
 *   load, fxb_meter_enable): the list calls do not change it - a host that resets a voice by list knows when it did.  Neither do
 *   they change instance state, gains, taps, tracks, code or any other counter.
 * FXB_INFO_METER_SELECTS / _LIST_READS / _LIST_RESETS count the calls that launched, summed over shards. */
#define FXB_METER_ENERGY     0
#define FXB_METER_PEAK       1
#define FXB_METER_FULL_SCALE 2
#define FXB_METER_NONFINITE  3
#define FXB_METER_BELOW (1u << 0)   /* select V < threshold instead of V >= threshold */
int64_t fxb_meter_select(fxb_handle* h, int stat, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags);
int fxb_meter_read_list(fxb_handle* h, const int64_t* list, int64_t count, double* energy, float* peak, uint32_t* full_scale, uint32_t* nonfinite, int reset);
int fxb_meter_reset_list(fxb_handle* h, const int64_t* list, int64_t count);
/* Target meters: the error of every instance against a reference signal, on the device.  A parameter sweep (FXB_BUS_SHARED_IN: one
 * signal through N instances that differ in their controls) asks which setting comes closest to a wanted response; with a target
 * set, the meter launch of every block also accumulates the squared error and the cross product against it, and three queries
 * bring back the verdict - never the [S][C][N] output words.  With no target set nothing changes: the same kernel, the same
 * arguments, no allocation.
 *
 * The definition.  fxb_meter_set_target(h, target, n_samples, group, flags):
 *   `target` is host memory [n_samples][num_channels][G], with G = ceil(N / group) and 1 <= group.  Instance n (global) is
 *   compared with column n / group.  group == 1 gives one target per instance.  group >= N gives one target for all instances.
 *   The handle keeps a TARGET POSITION p, set to 0 by this call.  Each (channel c, instance n) has two further accumulators:
 *   `err` (fp64), +0.0 after a reset; `cross` (fp64), +0.0 after a reset.
 *   For every output word y of that column, in sample order, let q be the target position of that sample.  The target position
 *   of a sample is the handle's position when its block was QUEUED, plus the sample's index in the block.
 *     - Without FXB_METER_TARGET_LOOP, a sample with q >= n_samples changes neither accumulator.
 *     - With FXB_METER_TARGET_LOOP, q is taken mod n_samples.
 *     - Otherwise t = target[q][c][n / group] and ok = |y| < +Inf && |t| < +Inf.
 *     - If !ok, neither accumulator changes.  The existing `nonfinite` counter already says that y was bad.
 *     - If ok:
 *         d = (double)y - (double)t  (one rounding);
 *         e = d * d  (one rounding);
 *         err = err + e  (one rounding, never fused with the multiply);
 *         cross = cross + (double)y * (double)t  (the product of two fp32 values is exact; one rounding).
 *   The four existing accumulators are taken exactly as now, for every sample.  After a block of S samples the position is
 *   p + S.  With LOOP it is reduced mod n_samples.  Without LOOP it is not clamped.
 *   No accumulator can become NaN or infinite for finite fp32 inputs: |d| < 2^129, so e < 2^258.  That keeps `>=` and `<`
 *   complements in the select.
 *   The figures do not depend on how a stream is cut - blocks of 16 + 17 samples, the pieces of the bus scratch and of a large
 *   host block, the segments of an armed control track, the shards: the position advances per launch, beside the count of
 *   fxb_meter_samples.
 *
 * fxb_meter_set_target is synchronous and waits as fxb_sync does.  It allocates the target block on every shard, and the match
 *   rows (16 bytes per instance and channel, [channel]{err[nPad], cross[nPad]}) where there are none.  It copies the target,
 *   zeroes the match rows and sets p = 0.  A shard keeps only the target columns its instances use: floor(first / group) ..
 *   floor((first + n - 1) / group); shards therefore need NO alignment to `group`, unlike bus blocks.  All allocation for the
 *   feature happens here, never in a block.  On FX_E_MEMORY no new target is set on any shard and the handle stays usable (a
 *   target that was in force stays in force).  FX_E_ARG, with nothing changed, for: metering off; a null `target`;
 *   n_samples < 1; group < 1; an unknown flag bit; num_channels * G_shard * 4 >= 2^32 (the kernel uses a 32-bit row stride);
 *   n_samples * num_channels * G >= 2^31 words.
 * Resets.  fxb_meter_clear_target drops the target; so do fxb_meter_enable(h, 0) and a program load (fxb_load_file /
 *   fxb_load_text).  All three free the target block and the match rows.  fxb_meter_read(..., reset = 1) zeroes the match rows
 *   as well and leaves p alone.  fxb_meter_reset_list zeroes the listed columns of the match rows as well - a reused slot gets
 *   fresh meters, all of them - by a launch of its own (fx_match_zero) queued beside fx_meter_zero, inside the same event frame.
 * fxb_meter_target_seek: the position of the next queued block; host-side, no wait.  Accepts 0 <= pos <= n_samples; with LOOP,
 *   pos must be < n_samples.  FX_E_ARG when no target is set.
 * fxb_meter_target_pos: p, or FX_E_ARG when no target is set.
 * fxb_meter_read_match behaves as fxb_meter_read does, on the two new rows: [num_channels][N] by global instance, either
 *   pointer may be NULL; `reset` zeroes only the two new rows.  FX_E_ARG when no target is set.
 * V(n) for select and best.  v(c, n) is accumulator `stat` (FXB_MATCH_ERROR, FXB_MATCH_CROSS).
 *   V(n) = ((v(0,n) + v(1,n)) + v(2,n)) + v(3,n) over the handle's channels, in fp64, in channel order, starting from v(0,n).
 *   This is a sum, not the maximum of fxb_meter_select: an error over a stereo pair is a sum.  It is still one fixed sequence of
 *   IEEE operations.
 * fxb_meter_select_match: everything else is as fxb_meter_select, refusals included: the ordered compaction, FXB_METER_BELOW,
 *   cap and range rules, and shard concatenation.  `stat` must be 0 or 1.  FX_E_ARG when no target is set.  fxb_meter_select
 *   itself keeps refusing stat = 4.
 * fxb_meter_best: groups are those of the bus calls: group g is instances g * group .. min((g + 1) * group, N) - 1, and
 *   G = ceil(N / group).  winner[g] is the instance of group g with the smallest V, or with FXB_MATCH_LARGEST the largest.  Ties
 *   go to the smallest instance number.  value[g] is that V.  Either pointer may be NULL.  It is synchronous, and 16 * G bytes
 *   cross PCIe.  `group` need not equal the target's group.  Sharded handles: each shard answers for the parts of groups it
 *   owns, and the host joins partial winners by the same order; the result equals the single handle's.  FX_E_ARG for
 *   group < 1, an unknown flag, `stat` outside 0..1, or no target set.  One wavefront works on a group: groups below 64
 *   instances leave lanes idle - a known cliff, like the mix of small groups.
 * FXB_INFO_METER_TARGET_LAUNCHES counts the launches of the kernel fx_meter_target, FXB_INFO_METER_LAUNCHES those of fx_meter:
 *   a block is metered by one or the other.  FXB_INFO_METER_MATCH_SELECTS / _MATCH_BESTS count the calls that launched.  All
 *   are summed over shards. */
#define FXB_METER_TARGET_LOOP (1u << 0)
int     fxb_meter_set_target(fxb_handle* h, const float* target, int64_t n_samples, int64_t group, unsigned flags);
int     fxb_meter_clear_target(fxb_handle* h);
int     fxb_meter_target_seek(fxb_handle* h, int64_t pos);     /* position of the next queued block; host-side, no wait */
int64_t fxb_meter_target_pos(fxb_handle* h);
int     fxb_meter_read_match(fxb_handle* h, double* err, double* cross, int reset);       /* [C][N]; pointers may be NULL */
#define FXB_MATCH_ERROR 0
#define FXB_MATCH_CROSS 1
#define FXB_MATCH_LARGEST (1u << 1)
int64_t fxb_meter_select_match(fxb_handle* h, int stat, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags);
int     fxb_meter_best(fxb_handle* h, int stat, int64_t group, int64_t* winner, double* value, unsigned flags);
/* Level meters: an envelope that falls and a quiet-run count per instance, on the device.  The six accumulators above only grow
 * after a reset - `peak` is a running maximum - so they cannot say which voices have STOPPED sounding.  With the level mode on, the
 * meter launch of every block also takes two accumulators that fall as well as rise: a PPM-style level with instant attack and
 * exponential release, and the number of consecutive samples below a floor ("below -80 dB for 4 800 samples: the slot is free").
 * Both are sample-by-sample recurrences carried in device memory.  With the mode off nothing changes: the same kernels, the same
 * arguments, no allocation.
 *
 * The definition.  fxb_meter_set_level(h, release, floor, flags) turns the mode on.  `release` is an fp32 value, finite, with
 *   0 <= release <= 1; `floor` is an fp32 value, finite, with floor >= 0; `flags` must be 0.  Each (channel c, instance n) gets two
 *   further accumulators: `level` (fp32), +0.0f after a reset; `quiet` (uint32), 0 after a reset.  For every output word y of that
 *   column, in sample order, with fin and w exactly those of "Output meters":
 *       fin   = |y| < +Inf
 *       w     = fin ? |y| : +0.0f
 *       d     = level * release      (one fp32 multiply, one rounding, denormals kept, never fused with anything)
 *       level = max(w, d)            (both are non-negative and finite: the larger bit pattern)
 *       loud  = !fin || w >= floor   (fp32 compare; a NaN or an infinity is loud)
 *       quiet = loud ? 0 : (quiet == 0xFFFFFFFF ? quiet : quiet + 1)
 *   The four existing accumulators are taken exactly as now, for every sample; with a target set, `err` and `cross` are too.
 *   Consequences:
 *     - release = 1 makes `level` the running peak since the reset: it equals `peak` bit for bit.
 *     - release = 0 makes `level` the magnitude of the last sample (+0 where that sample is not finite).
 *     - floor = 0 turns the counter off: it stays 0.
 *     - A non-finite voice is never "quiet".  It is found with FXB_METER_NONFINITE.
 *     - With a release close to 1 the envelope of a silent voice can come to rest at a small denormal instead of 0, because
 *       x * release rounds back to x once x * (1 - release) is at most half a denormal step (with release = 0.999 it stops
 *       falling at the bit pattern 500, with 0.93 at 7).  Compare it with a threshold, never with 0.
 *     - The figures do not depend on how a stream is cut - blocks of 16 + 17 samples against 33, the pieces of the bus scratch
 *       and of a large host block, the segments of an armed control track, the shards.
 *
 * fxb_meter_set_level: the first call waits as fxb_sync does.  It allocates and zeroes the level rows on every shard - per
 *   channel level f32 [nPad], then quiet u32 [nPad], a block of their own: 8 bytes per instance and channel.  Every shard is asked
 *   before any shard changes, so FX_E_MEMORY leaves the mode off everywhere and the handle usable.  All allocation for the feature
 *   happens here, never in a block.  A call while the mode is on changes only the two parameters, for blocks queued after it, and
 *   keeps the accumulators; it does not wait.  The parameters travel by value in each launch's arguments.  FX_E_ARG, with nothing
 *   changed, for: metering off; a NaN, infinite or out-of-range `release`; a NaN, infinite or negative `floor` (-0.0 is taken as
 *   0, for both); a non-zero flag.
 * Resets.  fxb_meter_clear_level and fxb_meter_enable(h, 0) free the rows.  A program load zeroes the rows and keeps the mode and
 *   its parameters, as it does for the four accumulators.  fxb_meter_read(..., reset = 1) zeroes the level rows as well;
 *   fxb_meter_read_level(..., reset = 1) zeroes only the level rows.  fxb_meter_reset_list zeroes the listed columns of the level
 *   rows too - a reused slot gets fresh meters, all of them - by one more stores-only launch (fx_level_zero) queued beside
 *   fx_meter_zero / fx_match_zero, inside the same event frame.  Instance copy, reset, save and load leave the level rows alone,
 *   as they leave every meter alone.
 * fxb_meter_get_level: the two parameters in force (either pointer may be NULL); FX_E_ARG while level meters are off.
 * fxb_meter_read_level / fxb_meter_read_level_list are fxb_meter_read / fxb_meter_read_list on the two new rows:
 *   [num_channels][N] and [num_channels][count] by (global) instance, either pointer may be NULL, synchronous.  A list may repeat
 *   an instance unless reset != 0; with reset, one lane of one launch reads and zeroes the same column.  The refusals are the
 *   same; FX_E_ARG while level meters are off.
 * fxb_meter_select_level: FXB_LEVEL_ENVELOPE: V(n) = the maximum over the channels of (double)level.  FXB_LEVEL_QUIET: V(n) = the
 *   MINIMUM over the channels of (double)quiet - a voice has been quiet for k samples only if every channel has.  Everything else
 *   is fxb_meter_select's: the ordered compaction without atomics, FXB_METER_BELOW, the cap, range and NaN-threshold rules, shard
 *   concatenation, cap == 0 as a count query.  `stat` outside 0..1 is FX_E_ARG; so are level meters off.  fxb_meter_select and
 *   fxb_meter_select_match keep their own `stat` ranges.
 * FXB_INFO_METER_LEVEL_LAUNCHES counts the meter launches that took the level rows (fx_meter_level, fx_meter_target_level).
 *   FXB_INFO_METER_LAUNCHES keeps counting the meter launches of blocks without a target, FXB_INFO_METER_TARGET_LAUNCHES those
 *   with one, whichever kernel ran: a block is still metered by exactly one launch.  FXB_INFO_METER_LEVEL_SELECTS /
 *   _LEVEL_LIST_READS count the calls that launched.  All are summed over shards. */
#define FXB_LEVEL_ENVELOPE 0
#define FXB_LEVEL_QUIET    1
int     fxb_meter_set_level(fxb_handle* h, float release, float floor, unsigned flags);
int     fxb_meter_clear_level(fxb_handle* h);
int     fxb_meter_get_level(fxb_handle* h, float* release, float* floor);        /* FX_E_ARG while level meters are off */
int     fxb_meter_read_level(fxb_handle* h, float* level, uint32_t* quiet, int reset);          /* [C][N]; pointers may be NULL */
int     fxb_meter_read_level_list(fxb_handle* h, const int64_t* list, int64_t count, float* level, uint32_t* quiet, int reset); /* [C][count] */
int64_t fxb_meter_select_level(fxb_handle* h, int stat, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags);
/* Meter ranks: the K quietest, loudest or closest voices, chosen on the device.  The selects answer "which voices pass this
 * threshold" and fxb_meter_best "which one voice of each group is closest"; a rank answers the question a voice pool asks when it
 * is full (a note-on arrives, no voice is below the floor: which K have the lowest envelope, whatever it is?), a fitting loop after
 * every sweep (the K best candidates of the whole range) and a diagnostic (the ten loudest).  It is an order statistic, and the
 * answer is K numbers - never the rows of every instance and a sort on the host.
 *
 * The definition.  fxb_meter_rank, fxb_meter_rank_match and fxb_meter_rank_level take (h, stat, k, threshold, first, n_range,
 *   list, value, flags):
 *   - V(n) is exactly the V(n) of the select of the same family, taken by the same device code: for the meter stats the fp64
 *     maximum over the channels; for the match stats the fp64 sum in channel order, starting from v(0,n); for FXB_LEVEL_ENVELOPE
 *     the maximum over the channels; for FXB_LEVEL_QUIET the minimum over the channels.
 *   - Candidates are the instances n in first .. first + n_range - 1 that the select would match: V(n) >= threshold, or with
 *     FXB_METER_BELOW V(n) < threshold.  threshold = -Inf without BELOW takes the whole range.  M is the number of candidates.
 *   - Candidates are ordered by the total order (V, n): V ascending as real numbers, so -0.0 equals +0.0, and ties go to the
 *     smaller instance number.  With FXB_METER_LARGEST the order is V descending, ties still to the smaller instance number.
 *   - The call writes the first R = min(M, k) candidates of that order to list[0..R-1] in rank order.  Their V goes to
 *     value[0..R-1] when `value` is not NULL.  Neither array is touched beyond R.  The call returns M, as the selects do.
 *   - k == 0 is a count query, and n_range == 0 returns 0 without a launch.
 *   - No V is ever NaN (argued per family above), so the order is total.
 *   - The call is synchronous and changes nothing, like fxb_meter_select.  It covers a list reset still in flight.
 * Refusals.  FX_E_ARG, with nothing launched: everything the matching select refuses (the mode off - metering, the target, the
 *   level meters -, `stat` out of the family's range, a NaN threshold, the range rules, an unknown flag bit); k < 0; a NULL `list`
 *   with k > 0.  FX_E_MEMORY when the staging cannot be allocated: it is grown on demand, freed with the handle and sized by
 *   min(k, n_range) - 16 bytes per pair - plus 16 bytes per chunk of 256 instances and a fixed 16 KB of histograms; nothing has
 *   changed afterwards.
 * The device side is a selection, not a sort: a radix select over 64-bit keys (V + 0.0 with the sign-flip transform, complemented
 *   for LARGEST) finds the key of the k-th candidate in eight passes of eight bits, then the count / scan / emit pattern of the
 *   selects writes the winners - a tie at the k-th key goes to the first of the equals by instance number.  The number of launches
 *   (eleven kernels behind one memset; ten for a count query) depends neither on N nor on the data; there is one wait, at the end;
 *   min(M, k) * 16 bytes and four words cross PCIe (for M < k: min(k, 4 096) pairs, so that the wait stays one).  The only atomics
 *   are integer adds into histogram bins, whose sums no order can change: the same bits run to run.
 * Sharded handles: each shard answers for its part of the range with its own first min(k, M_s) pairs, and the host merges the parts
 *   under the same total order on global instance numbers; the result equals the single handle's word for word.  A shard whose
 *   part is empty launches nothing.  The return value is the sum of the M_s.
 * FXB_INFO_METER_RANKS / _MATCH_RANKS / _LEVEL_RANKS count the calls that launched, summed over shards. */
#define FXB_METER_LARGEST (1u << 1)   /* same bit as FXB_MATCH_LARGEST */
int64_t fxb_meter_rank(fxb_handle* h, int stat, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags);
int64_t fxb_meter_rank_match(fxb_handle* h, int stat, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags);   /* stat: FXB_MATCH_ERROR / _CROSS; needs a target */
int64_t fxb_meter_rank_level(fxb_handle* h, int stat, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags);   /* stat: FXB_LEVEL_ENVELOPE / _QUIET; needs level meters */
/* Tone meters: per-instance power at K probe frequencies, on the device.  Every other figure the device keeps per instance is
 * broadband; the tone meters say where in the spectrum the energy sits - the gain of every variant of a sweep at a handful of
 * frequencies, the voices that ring at a note's pitch or carry hum, the variants of a feedback network that build up at a
 * resonance.  The answer is a Goertzel recurrence per (tone, channel, instance): two fp64 words of state and three fp64 operations
 * per sample, no table and no position - the phase lives in the state - so the figures do not depend on how a stream is cut.  With
 * the mode off nothing changes: the same kernels, the same arguments, no allocation.
 *
 * The definition.  fxb_meter_set_tones(h, n_tones, coeff, flags) turns the mode on.  1 <= n_tones <= FXB_METER_MAX_TONES;
 *   coeff[k] is a finite double with -2 <= coeff[k] <= 2 (-0.0 is taken as +0.0); `flags` must be 0.  The caller computes
 *   c = 2 cos(2 pi f / fs); the library takes the double as given, so no libm call is part of the definition.  Each (tone k,
 *   channel c, instance n) gets two fp64 words s1 and s2, +0.0 after a reset.  For every output word y of that column, in sample
 *   order, with fin exactly that of "Output meters":
 *       x  = fin ? (double)y : +0.0     (the signed word; a NaN or an infinity contributes nothing, but time still passes)
 *       p  = c * s1                     (one fp64 multiply)
 *       q  = x + p                      (one fp64 add)
 *       s0 = q - s2                     (one fp64 subtract)
 *       s2 = s1 ;  s1 = s0
 *   Nothing is fused: the library is built with -ffp-contract=off and the contract depends on it.  The figure is
 *       P = (s1*s1 + s2*s2) - (c*s1)*s2
 *   five fp64 operations in exactly that order.  After n samples of A sin(2 pi k t / n + phi) probed at bin k (c = 2 cos(2 pi k /
 *   n)), P is about (A n / 2)^2.  With |c| <= 2 the impulse response of the recurrence is bounded by its index, so |s1| <=
 *   n (n + 1) / 2 * max|y|: from fp32 inputs no reachable sample count makes a word non-finite or P a NaN (the ranks' rule "no V
 *   is ever NaN" rests on this), and that is why coefficients beyond +-2 are refused.  P may come out a few ulps negative; it is
 *   ordered as the real number it is.  The four existing accumulators, the match rows and the level rows are taken exactly as
 *   without the mode.
 *
 * fxb_meter_set_tones needs metering on (FX_E_ARG otherwise).  Every successful call waits as fxb_sync does and takes the rows
 *   into force zeroed: accumulators of other coefficients mean nothing.  The tone block - a header with the coefficients, then
 *   [num_channels][n_tones][2][nPad] doubles - is allocated on every shard before any shard changes: FX_E_MEMORY leaves the mode as
 *   it was everywhere.  All allocation of the feature happens here, never in a block.  A refusal changes nothing.  While the mode
 *   is on, every block's meter launch is followed by one launch of fx_meter_tone on the same stream, with the coefficients by value.
 * fxb_meter_get_tones: the mode in force - *n_tones and coeff[0 .. n_tones - 1] (either pointer may be NULL; coeff must have room
 *   for FXB_METER_MAX_TONES); FX_E_ARG while the mode is off.  fxb_meter_clear_tones and fxb_meter_enable(h, 0) free the rows.
 * Resets.  fxb_meter_read(..., reset = 1) and a program load zero the tone rows with the others and keep the mode.
 *   fxb_meter_reset_list zeroes the listed columns by one more stores-only launch (fx_tone_zero) inside the same event frame as
 *   its siblings.  Instance copy, reset, save, load and the record bank leave the tone rows alone; the state image does not hold them.
 * fxb_meter_read_tones: s1, s2, power are [n_tones][num_channels][N] doubles by (global) instance; any of the three may be NULL.
 *   Waits as fxb_sync does.  reset != 0 zeroes only the tone rows.  `power` is P, computed by the one function that defines it.
 * fxb_meter_read_tones_list: [n_tones][num_channels][n_list], with the list rules of fxb_meter_read_level_list: a list may repeat
 *   an instance unless reset != 0; with reset, the lane that has read a column stores its zeros.
 * fxb_meter_select_tone / fxb_meter_rank_tone: fxb_meter_select's and fxb_meter_rank's contracts over V(n) = the maximum over the
 *   channels of P(tone, c, n).  `tone` outside 0 .. n_tones - 1 is FX_E_ARG; so is the mode off.
 * FXB_INFO_METER_TONE_LAUNCHES counts the launches of fx_meter_tone; FXB_INFO_METER_TONE_SELECTS / _TONE_LIST_READS / _TONE_RANKS
 *   the calls that launched.  All are summed over shards. */
#define FXB_METER_MAX_TONES 8
int     fxb_meter_set_tones(fxb_handle* h, int n_tones, const double* coeff, unsigned flags);
int     fxb_meter_get_tones(fxb_handle* h, int* n_tones, double* coeff);           /* FX_E_ARG while tone meters are off */
int     fxb_meter_clear_tones(fxb_handle* h);
int     fxb_meter_read_tones(fxb_handle* h, double* s1, double* s2, double* power, int reset);     /* [K][C][N]; pointers may be NULL */
int     fxb_meter_read_tones_list(fxb_handle* h, const int64_t* list, int64_t n_list, double* s1, double* s2, double* power, int reset); /* [K][C][n_list] */
int64_t fxb_meter_select_tone(fxb_handle* h, int tone, double threshold, int64_t first, int64_t n_range, int64_t* list, int64_t cap, unsigned flags);
int64_t fxb_meter_rank_tone(fxb_handle* h, int tone, int64_t k, double threshold, int64_t first, int64_t n_range, int64_t* list, double* value, unsigned flags);
int fxb_sync(fxb_handle* h);
/* executed instructions (reference counting: END and SKIP count, skipped ones do not):
 * summed over all instances / of one instance */
int64_t fxb_instruction_counter(fxb_handle* h);
int64_t fxb_instruction_counter_i(fxb_handle* h, int64_t instance);
/* OR of the per-instance "outside the parity domain" flags (0 = the whole batch stayed
 * inside the domain where the reference's behaviour is defined) */
uint32_t fxb_ood_flags(fxb_handle* h);
/* front-end results, as fx_* */
int fxb_error_count(fxb_handle* h);
const char* fxb_error_desc(fxb_handle* h, int i);
int fxb_error_row(fxb_handle* h, int i);
int fxb_control_count(fxb_handle* h);
const char* fxb_control_at(fxb_handle* h, int i);
int fxb_meta_get(fxb_handle* h, const char* key, char* buf, int buflen);
int fxb_ready(fxb_handle* h);
const char* fxb_last_error(fxb_handle* h);
/* HIP-event duration (ms) of the most recent interpreter-kernel launch, measured on the
 * stream it ran on; <0 if none.  Implies a sync on that stream.  While metering is on (fxb_meter_enable) the
 * duration covers the launch and the meter launch behind it. */
float fxb_last_kernel_ms(fxb_handle* h);

/* introspection of the lowered program (what the kernel actually runs) */
enum {
    FXB_INFO_NUM_INSTRUCTIONS = 0, /* reference instruction count, END included           */
    FXB_INFO_NUM_REGISTERS = 1,    /* reference register count                            */
    FXB_INFO_NUM_LANE_REGS = 2,    /* registers kept per instance (LDS rows)              */
    FXB_INFO_NUM_UNIFORM_REGS = 3, /* registers folded into the opcode stream             */
    FXB_INFO_LDS_BYTES_PER_WG = 4,
    FXB_INFO_WAVES_PER_WG = 5,
    FXB_INFO_NUM_MICROOPS = 6,     /* records in the device opcode stream                 */
    FXB_INFO_ITRAM_SLOTS = 7,      /* allocated slots per instance                        */
    FXB_INFO_XTRAM_SLOTS = 8,
    FXB_INFO_TRAM_OPS = 9,         /* delay reads+writes per sample (static)              */
    FXB_INFO_MULTIPASS = 10,       /* 1 if END can be skipped (generic pass loop in use)  */
    FXB_INFO_NUM_SHADOWED = 11,    /* instructions that can sit in a SKIP shadow          */
    FXB_INFO_NUM_CCR_LIVE = 12,    /* instructions whose CCR write is observable          */
    FXB_INFO_DEVICE = 13,
    FXB_INFO_GRID = 14,            /* workgroups of the last launch                       */
    FXB_INFO_INST_PER_LANE = 15,   /* instances one lane steps (kernel variant)           */
    FXB_INFO_KERNEL = 16,          /* 0 = HIP C++ kernel; hand-written gfx950 interpreter: 1 = register file in LDS,
                                      2..8 = register file in VGPRs (64/72/80/96/128/168/256-VGPR build);
                                      9..15 = program translated to gfx950 code, same seven VGPR builds */
    FXB_INFO_NUM_ROWS = 17,        /* rows of the per-instance register file               */
    FXB_INFO_XLATE_CODE_BYTES = 18,/* translated program: bytes of machine code (both streams), else 0 */
    FXB_INFO_XLATE_INLINED = 19,   /* records of the steady stream turned into straight-line code */
    FXB_INFO_XLATE_CALLED = 20,    /* records of the steady stream that call an interpreter handler */
    FXB_INFO_XLATE_UNSATURATED = 21,/* saturating instructions translated without a saturation (result provably in [-1, 1]) */
    FXB_INFO_XLATE_VALU = 22,       /* translated program: vector-ALU instructions per wavefront and sample period (the steady loop wavefronts start in) */
    FXB_INFO_XLATE_VALU_SLOW = 23,  /* ... those of the ~4-clock issue class (conversions, min/max/med3, compares, fp64, SGPR sources) */
    FXB_INFO_XLATE_VALU_CLOCKS = 24,/* ... modelled SIMD issue clocks of all of them per wavefront and sample period */
    FXB_INFO_XLATE_VGPR_CONSTANTS = 25, /* uniform constants the translated code keeps in spare VGPRs */
    FXB_INFO_XLATE_BUILDS = 26,    /* translations (code generation + module load) on the CALLER's thread since the handle was created: each one
                                      held a process call up for a few milliseconds */
    FXB_INFO_CODE_CACHE_HITS = 27, /* changes of code that were a pointer swap: the shape (block-length class, set of registers with rows, compiled-in
                                      values) had been generated before - by an earlier call or ahead of time by the builder thread */
    FXB_INFO_CODE_CACHED = 28,     /* generated code objects the handle holds (the one in force included) */
    FXB_INFO_XLATE_CODE_HASH = 30, /* fingerprint (63 bits) of the code object in force, 0 when the program is not translated: what a profile of a
                                      launch is a profile of (fxp_code_hash computes the same without a device) */
    FXB_INFO_STAGE_TRIALS = 31,    /* launches whose time went into the choice of the stage count (options the cost model cannot tell apart are timed
                                      on the caller's own blocks; FX_STAGES_TUNE=0 turns that off, FX_STAGES=n pins the count) */
    FXB_INFO_XLATE_BACKGROUND_BUILDS = 29, /* translations on the handle's builder thread (ahead of time: the variant with the declared controls in
                                      rows, the lean variant, code for another class of block lengths); FX_BUILDER=0 in the environment turns the thread off */
    FXB_INFO_CONTROL_ROWS = 32,    /* declared controls that have a register row in the code in force: 0 until the host moves one (their values are
                                      folded into the code), then all of them (one change of code for the whole panel, generated ahead of time), then
                                      - a few blocks later, a pointer swap - only the ones that have been written lately (within 8192 sample periods;
                                      the others go back into the code, where a constant is cheaper than a row: e.g. INTERP with a constant X).  Same
                                      results in all three. */
    FXB_INFO_HOST_STAGED_BLOCKS = 33,  /* host blocks that went through staging copies since creation (summed over shards) */
    FXB_INFO_HOST_INPLACE_BLOCKS = 34, /* host blocks processed on the caller's pinned buffers in place (summed over shards) */
    FXB_INFO_BUS_BLOCKS = 35,          /* bus blocks (fxb_process_block_bus* with a flag set) since creation (summed over shards) */
    FXB_INFO_METER_LAUNCHES = 36,      /* launches of the output-meter kernel (fxb_meter_enable) since creation (summed over shards) */
    FXB_INFO_IMAJOR_BLOCKS = 37,       /* instance-major blocks since creation (summed over shards) */
    FXB_INFO_INSTANCE_WORDS = 38,      /* W: 32-bit words of one instance's record (state rows + iTRAM slots + xTRAM slots) */
    FXB_INFO_INSTANCE_GATHERS = 39,    /* launches of the kernel fx_inst_gather - by fxb_copy_instances and fxb_save_instances - since creation (summed over shards) */
    FXB_INFO_INSTANCE_SCATTERS = 40,   /* launches of the kernel fx_inst_scatter - by copy, reset and load - since creation (summed over shards) */
    FXB_INFO_BUS_GAIN_BLOCKS = 41,     /* bus blocks mixed with gains (fxb_bus_set_gains) since creation (summed over shards) */
    FXB_INFO_BUS_TAP_BLOCKS = 42,      /* bus blocks that delivered taps (fxb_process_block_bus_tap* with a tap_out) since creation (summed over shards) */
    FXB_INFO_BUS_SEND_BLOCKS = 43,     /* bus blocks that delivered sends (fxb_process_block_bus_aux* with an aux_out) since creation (summed over shards) */
    FXB_INFO_BUS_FEED_BLOCKS = 44,     /* bus blocks filled by feeds (fxb_process_block_bus_feed*) since creation (summed over shards) */
    FXB_INFO_INSTANCE_RINGS = 45,      /* bit 0: iTRAM, bit 1: xTRAM is a ring in which a record can be rotated (fxb_load_instances_rotated); 0 without delay lines */
    FXB_INFO_XLATE_QUIET = 47,      /* 1 when the code in force has a quiet loop (fxp_translate stream 5): its wavefronts start there, and
                                      FXB_INFO_XLATE_VALU / _VALU_SLOW / _VALU_CLOCKS / _UNSATURATED describe that loop */
    FXB_INFO_XLATE_QUIET_LEFT = 48, /* wavefronts of the last launch that left the quiet loop - for the steady fast loop (a lane above its bound at
                                      the head of a sample) or for the exact stream (a non-finite value); waits for that launch (summed over shards) */
    FXB_INFO_INSTANCE_ROTATIONS = 46,  /* launches of the kernel fx_inst_scatter_rot - by fxb_load_instances_rotated - since creation (summed over shards) */
    FXB_INFO_GAIN_LIST_SETS = 49,      /* launches of the kernel fx_gain_scatter - by fxb_bus_set_gains_list / _send_gains_list / _feed_gains_list - since creation (summed over shards) */
    FXB_INFO_REGISTER_LIST_SETS = 50,  /* launches of the kernel fx_reg_scatter - by fxb_set_registers_list - since creation (summed over shards) */
    FXB_INFO_REGISTER_LIST_GETS = 51,  /* launches of the kernel fx_reg_gather - by fxb_get_registers_list - since creation (summed over shards) */
    FXB_INFO_XLATE_SUM_GROUPS = 52,    /* sum groups of the quiet loop in force (fxp_translate stream 6; 0: the loop has none, or there is no loop): chains of
                                          saturating sums on one accumulator that the loop tests once per group instead of saturating every link */
    FXB_INFO_XLATE_SUM_LINKS = 53,     /* ... and the saturating instructions inside those groups */
    FXB_INFO_XLATE_QUIET_REPAIRS = 54, /* how often the last launch re-did a sum group with its saturations (a lane's partial sum above the group's
                                          threshold), summed over wavefronts; a repair does not leave the loop; waits for that launch (summed over shards) */
    FXB_INFO_TRAM_LIST_SETS = 55,      /* launches of the kernel fx_tram_scatter - by fxb_set_tram_list - since creation (summed over shards) */
    FXB_INFO_TRAM_LIST_GETS = 56,      /* launches of the kernel fx_tram_gather - by fxb_get_tram_list - since creation (summed over shards) */
    FXB_INFO_METER_SELECTS = 57,       /* calls of fxb_meter_select that launched (fx_meter_count / _scan / _emit) since creation (summed over shards) */
    FXB_INFO_METER_LIST_READS = 58,    /* calls of fxb_meter_read_list that launched (fx_meter_gather) since creation (summed over shards) */
    FXB_INFO_METER_LIST_RESETS = 59,   /* calls of fxb_meter_reset_list that launched (fx_meter_zero) since creation (summed over shards) */
    FXB_INFO_METER_TARGET_LAUNCHES = 61, /* launches of the kernel fx_meter_target - the meter launch of a block while a target is set (fxb_meter_set_target) - since creation (summed over shards) */
    FXB_INFO_METER_MATCH_SELECTS = 62,   /* calls of fxb_meter_select_match that launched (fx_match_count / fx_meter_scan / fx_match_emit) since creation (summed over shards) */
    FXB_INFO_METER_MATCH_BESTS = 63,     /* calls of fxb_meter_best that launched (fx_meter_best) since creation (summed over shards) */
    FXB_INFO_METER_LEVEL_LAUNCHES = 64,  /* meter launches that took the level rows (fx_meter_level, fx_meter_target_level) since creation (summed over shards) */
    FXB_INFO_METER_LEVEL_SELECTS = 65,   /* calls of fxb_meter_select_level that launched (fx_level_count / fx_meter_scan / fx_level_emit) since creation (summed over shards) */
    FXB_INFO_METER_LEVEL_LIST_READS = 66, /* calls of fxb_meter_read_level_list that launched (fx_level_gather) since creation (summed over shards) */
    FXB_INFO_BANK_SLOTS = 67,            /* slots of the record bank (fxb_bank_create), 0 without one; every shard holds them all: not summed */
    FXB_INFO_BANK_STORES = 68,           /* launches of the kernel fx_bank_gather - by fxb_bank_store - since creation (summed over shards) */
    FXB_INFO_BANK_RECALLS = 69,          /* launches of the kernel fx_bank_scatter_rot - by fxb_bank_recall, refused ones included - since creation (summed over shards) */
    FXB_INFO_BANK_BYTES = 70,            /* device memory of the bank's slots: n_slots * W * 4 (summed over shards: each holds a copy) */
    FXB_INFO_TRACK_LIST_EXPANDS = 60,  /* blocks that launched the expansion of list schedules (fx_track_hold, fx_track_scatter): once per block and shard, summed over shards */
    FXB_INFO_METER_RANKS = 71,           /* calls of fxb_meter_rank that launched (fx_rank_hist / _count / _scan / _emit) since creation (summed over shards) */
    FXB_INFO_METER_MATCH_RANKS = 72,     /* calls of fxb_meter_rank_match that launched since creation (summed over shards) */
    FXB_INFO_METER_LEVEL_RANKS = 73,     /* calls of fxb_meter_rank_level that launched since creation (summed over shards) */
    FXB_INFO_METER_TONE_LAUNCHES = 74,   /* launches of the kernel fx_meter_tone - behind the meter launch of a block while tone meters are on (fxb_meter_set_tones) - since creation (summed over shards) */
    FXB_INFO_METER_TONE_SELECTS = 75,    /* calls of fxb_meter_select_tone that launched (fx_tone_count / fx_meter_scan / fx_tone_emit) since creation (summed over shards) */
    FXB_INFO_METER_TONE_LIST_READS = 76, /* calls of fxb_meter_read_tones_list that launched (fx_tone_gather) since creation (summed over shards) */
    FXB_INFO_METER_TONE_RANKS = 77       /* calls of fxb_meter_rank_tone that launched since creation (summed over shards) */
};
int64_t fxb_info(fxb_handle* h, int what);
/* Which tier runs the program as it stands, in words - "translated to gfx950 code (fx_xlate_v128, 8 stages)", "interpreter
 * (fx_interp_v96): <why there is no translation>" (a SKIP that can jump over END: passes over the program; a register file above
 * 224 rows; controls that keep moving ...), "HIP C++ kernel (1 instance(s) per lane): <why no assembly tier takes the program>"
 * (a register file beyond every build, a literal LOG / EXP table number outside 0..31 ...) - so that a host that finds
 * FXB_INFO_KERNEL below 9 can say why.  Copies at most buflen-1 characters, returns the note's length
 * (negative FX_E_*).  Of shard 0 for a multi-device handle (every shard runs the same code).  Nothing in the reference. */
int fxb_tier_note(fxb_handle* h, char* buf, int buflen);


/* ------------------------------------------------------------------ front-end only (no device)
 * The host-side loader and lowering, usable without a GPU: what the .da text became.
 * Mirrors the reference's private model (include/FX8010.h:167-194) for inspection and tests. */
typedef struct fxp_handle fxp_handle;
fxp_handle* fxp_create(int num_channels);
void fxp_destroy(fxp_handle* h);
int fxp_set_option(fxp_handle* h, unsigned option, int on);
int fxp_load_file(fxp_handle* h, const char* path);
int fxp_load_text(fxp_handle* h, const char* text);
int fxp_num_registers(fxp_handle* h);
const char* fxp_register_name(fxp_handle* h, int i);
int fxp_register_type(fxp_handle* h, int i);    /* reference RegisterType numbering */
int fxp_register_ioindex(fxp_handle* h, int i);
float fxp_register_value(fxp_handle* h, int i);
int fxp_num_instructions(fxp_handle* h);
/* out8 = opcode (reference Opcode numbering), R, A, X, Y, hasInput, hasOutput, hasNoise */
void fxp_instruction(fxp_handle* h, int i, int out8[8]);
int fxp_itram_size(fxp_handle* h);
int fxp_xtram_size(fxp_handle* h);
int fxp_error_count(fxp_handle* h);
const char* fxp_error_desc(fxp_handle* h, int i);
int fxp_error_row(fxp_handle* h, int i);
int fxp_control_count(fxp_handle* h);
const char* fxp_control_at(fxp_handle* h, int i);
int fxp_meta_get(fxp_handle* h, const char* key, char* buf, int buflen);
int fxp_ready(fxp_handle* h);
/* LOG (kind 0) / EXP (kind 1) table of one exponent: 64 doubles (reference FX8010.cpp:63-105) */
const double* fxp_lut(int kind, int exponent);
/* lower for the device with the registers' initial values; 0 or FX_E_PROGRAM.  fxp_lower_info
 * takes the FXB_INFO_* selectors that describe the lowering. */
int fxp_lower(fxp_handle* h);
int64_t fxp_lower_info(fxp_handle* h, int what);
/* Translate the loaded program to gfx950 machine code as the batch path would (no device needed), for the VGPR
 * build with `vgprs` registers (64/72/80/96/128/168/256; 0 = the smallest build that holds the program).
 * stream: 0 = steady fast, 1 = steady exact, 2 = last-sample fast, 3 = last-sample exact (fast streams assume a
 * finite register file and leave for the exact one when a non-finite value appears; a program with a non-finite
 * uniform operand has no fast streams: size 0); 4 = run-once code (LDS tables).  Returns the code size in bytes (negative FX_E_* when the program
 * cannot be translated, see fxp_last_error) and copies at most `cap` bytes of code and at most listing_cap-1
 * characters of the assembler listing (one instruction per line). */
int64_t fxp_translate(fxp_handle* h, int vgprs, int stream, void* code, int64_t cap, char* listing, int64_t listing_cap);
/* stream 5 = the steady QUIET loop of an unstaged program that has one (size 0 otherwise): the steady fast stream without the
 * saturations that cannot fire while the rows checked at the head of each sample stay inside their bounds; wavefronts start
 * there and leave for the steady fast loop when a lane fails the check (FXB_INFO_XLATE_QUIET, FXB_INFO_XLATE_QUIET_LEFT).
 * fxp_quiet_plan describes it (read-only): int32 words
 *   [0] a quiet loop is generated  [1] the program is eligible  [2] saturating records  [3] saturations the fast stream drops
 *   [4] ... the quiet loop drops  [5] vector instructions of the head check  [6] C = checked rows  [7] D = dropped records
 *   [8] R = records of the steady stream; then C x {register-file row, register index or -1, bound as float bits},
 *   D record indices, R x 8 record words; then Z and Z record indices: the records whose add of a uniform +0 the quiet loop
 *   does not emit because the other side cannot be -0 (ascending; no part of the counts above); then G and L: the sum groups of
 *   the loop and the links in them (below), and G x {register-file row R of the chain, threshold T as float bits, N = links of
 *   the group, flags (1 first, 2 last group of its chain, 4 the chain's start is an operand of the test), VGPR that holds the
 *   value in front of the group, running bound of the chain's start as float bits, N x {record index, 1 = its sum is an
 *   operand of the test (watched), 1 = the addend is subtracted, register-file row that is the addend or -1 for a product,
 *   VGPR the addend is kept in or -1 for the row itself, VGPR of its sum, running bound of the addend as float bits}}.
 * stream 6 = the quiet loop WITH sum groups (size 0 where the plan has none - no chain, or a VGPR build without spare registers):
 * the loop of stream 5 in which the kept saturations of an accumulator chain - R = sat(R +- addend), link after link - are
 * tested once per group of links (max |watched sums| against T) and re-done, in a stub behind the loop, only when a lane with an
 * instance is above T.  Where stream 6 exists it is what the device runs in place of stream 5 (FXB_INFO_XLATE_SUM_GROUPS,
 * _SUM_LINKS, _QUIET_REPAIRS); stream 5 reads the same either way.
 * Copies at most `cap` words, returns the number of words there are (negative FX_E_*); fxp_last_error says why a program has
 * no quiet loop. */
int64_t fxp_quiet_plan(fxp_handle* h, int vgprs, int32_t* out, int64_t cap);
/* ... with `key` among the registers that can have a control track (fxb_set_register_track): the code fxp_translate then
 * returns is what a batch runs after a track has been armed for that register.  0 found, 1 not found, FX_E_ARG beyond 16. */
int fxp_track_register(fxp_handle* h, const char* key);
/* The same for the program cut into (at most) `stages` stages run by the wavefronts of one workgroup - what the batch path
 * generates for small batches (fx_xlate.hpp StageInfo): the code of stream `stream` of stage `stage` (stream 4: the shared
 * run-once code).  *stages_out = the number of stages the program was cut into (1: not cut - the call then returns the
 * unstaged code and fxp_last_error says why); info (optional, info_cap ints): per cut {first record of the next stage, rows
 * handed over}, then the LDS bytes of a workgroup, the number of register-file rows and, per row, the stage that stores it. */
int64_t fxp_translate_staged(fxp_handle* h, int vgprs, int stages, int stage, int stream, void* code, int64_t cap, char* listing, int64_t listing_cap,
                             int* stages_out, int* info, int info_cap);
/* Fingerprint (63 bits, >= 0; negative FX_E_*) of the code object a batch would load for this program with its registers' initial
 * values: the `vgprs` build (64 ... 256), cut into at most `stages` stages (1: not cut; the default LDS budget and step length
 * of a small batch with long blocks), flags bit 0 = delay lines larger than the caches (non-temporal TRAM accesses), bit 1 =
 * the wavefronts of a SIMD take turns at the top priority (what a batch of two or more wavefronts per SIMD generates, on a build of
 * at most four wave slots: 128 registers and up).  Equals
 * fxb_info(FXB_INFO_XLATE_CODE_HASH) of a batch in that situation: tests and bench.py use it to tell whether a committed profile
 * still describes the code that is generated today. */
int64_t fxp_code_hash(fxp_handle* h, int vgprs, int stages, unsigned flags);
const char* fxp_last_error(fxp_handle* h);

/* library / device probe: number of HIP devices visible (0 if none), never throws */
int fxb_device_count(void);
const char* fxb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FX8010_AMD_H */
