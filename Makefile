# Build everything for MI355X (gfx950).  `make -j8` in the build container
# cross-compiles; the built .so / executables travel to the GPU box in-tree.
#
#   lz4-jpeg_amd/lz4jpeg/liblz4jpeg.so   product C-ABI library (HIP kernels)
#   lz4-jpeg_amd/bin/LZ4_seq, JPEG_seq    drop-in executables (file contract),
#                                         also as LZ4_seq.exe / JPEG_seq.exe
#   lz4-jpeg_amd/bin/LZ4_frame            file -> standard .lz4 frame on the GPU, -D back on the GPU, -d on the host (also LZ4_frame.exe)
#   lz4-jpeg_amd/bin/JPEG_dec             coefficients.jpr -> PNG (also JPEG_dec.exe)
#   lz4-jpeg_amd/bin/JPEG_sel             images or tile windows of a .jpr -> a new .jpr (also JPEG_sel.exe)
#   oracle/liboracle.so (+ oracle/_ref)   test-only CPU checker
#   lz4-jpeg_amd/build/liblz4r_chunk12.so test-only: the compressor alone, cut into
#                                         launch chunks of 2^12 blocks
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CC      ?= gcc
PKG     := lz4-jpeg_amd
CSRC    := $(PKG)/csrc
HOST    := $(PKG)/host
B       := $(PKG)/build
BIN     := $(PKG)/bin
HIPFLAGS := --offload-arch=$(ARCH) -O3 -ffp-contract=off -fno-strict-aliasing -fPIC -std=c++17 -Wall \
            -Wno-unused-result
# lz4r.hip (the compressor): the max-ILP machine scheduler, -0.3 % lz4_tiles and
# call time in three in-process A/B orders (tools/ab_inproc.py)
LZ4R_HIPFLAGS := -mllvm -amdgpu-sched-strategy=max-ilp
# lz4r_gpudec.hip (the block decoder): the max-memory-clause scheduler, -0.45 %
# (tools/ab_dec_inproc.py)
LZ4R_GPUDEC_HIPFLAGS := -mllvm -amdgpu-sched-strategy=max-memory-clause
CFLAGS_HOST := -O2 -fPIC -Wall -std=gnu11 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
LIB     := $(PKG)/lz4jpeg/liblz4jpeg.so
# test-only variant of lz4r.hip (self-contained: the compressor and its C ABI)
# with launch chunks of 2^12 blocks instead of 2^24, so that tests of a few MB
# cross chunk boundaries (tests/test_gpu_lz4_chunks.py); 2^12 = kPart, the
# smallest chunk the source accepts.  The product's flags plus the one define.
CHUNK12_LIB := $(B)/liblz4r_chunk12.so
CHUNK12_DEFINE := -DLZ4R_CHUNK_LOG2=12
CHUNK12_HIPFLAGS = $(HIPFLAGS) $(LZ4R_HIPFLAGS) $(CHUNK12_DEFINE)
HDRS    := include/lz4r.h include/jpegr.h include/lz4jpeg_compat.h include/lz4jpeg_synth.h \
           $(CSRC)/jpeg_tables.h $(CSRC)/jpeg_tables_dev.h \
           $(CSRC)/wave64.h $(CSRC)/lz4r_prof.h $(CSRC)/lz4r_layout.h $(CSRC)/lz4r_tile_lds.h \
           $(CSRC)/lz4r_tiles.h $(CSRC)/lz4r_matches.h $(CSRC)/lz4r_scan.h $(CSRC)/lz4r_emit.h \
           $(CSRC)/lz4r_frame.h $(HOST)/lz4f_xxh32.h \
           $(CSRC)/lz4r_dec_layout.h $(CSRC)/lz4r_dec_parse.h $(CSRC)/lz4r_dec_blocks.h \
           $(CSRC)/lz4r_dec_bare.h $(CSRC)/lz4r_dec_read.h $(CSRC)/lz4r_scratch.h \
           $(CSRC)/lz4f_parse.h $(CSRC)/lz4f_dec.h $(CSRC)/jpegr_pack_common.h \
           $(CSRC)/jpegr_entropy_common.h $(CSRC)/jpegr_decode_common.h $(CSRC)/jpegr_crop.h \
           $(CSRC)/jpegr_pixel.h $(CSRC)/jpegr_dct.h $(CSRC)/jpegr_recon.h $(CSRC)/jpegr_tensor_elem.h \
           $(CSRC)/jpegr_resize.h $(CSRC)/jpegr_dataset.h
OBJS    := $(B)/lz4r.o $(B)/lz4r_gpudec.o $(B)/lz4f_gpudec.o $(B)/lz4r_read.o $(B)/jpegr.o $(B)/jpegr_blocks.o \
           $(B)/jpegr_entropy.o $(B)/jpegr_pack.o $(B)/jpegr_stream.o $(B)/jpegr_stream_enc.o \
           $(B)/jpegr_thumb.o $(B)/jpegr_select.o $(B)/jpegr_resize.o \
           $(B)/synth.o $(B)/synth_dev.o \
           $(B)/lz4r_decode.o $(B)/lz4f_decode.o $(B)/compat.o $(B)/compat_lz4.o

all: lib bin oracle tools chunk12

lib: $(LIB)

bin: $(BIN)/LZ4_seq $(BIN)/JPEG_seq $(BIN)/LZ4_seq.exe $(BIN)/JPEG_seq.exe \
     $(BIN)/LZ4_par $(BIN)/JPEG_par $(BIN)/LZ4_par.exe $(BIN)/JPEG_par.exe \
     $(BIN)/JPEG_dec $(BIN)/JPEG_dec.exe $(BIN)/JPEG_sel $(BIN)/JPEG_sel.exe \
     $(BIN)/LZ4_frame $(BIN)/LZ4_frame.exe

$(CSRC)/jpeg_tables.h: $(CSRC)/gen_jpeg_tables.py
	python3 $< > $@

$(CSRC)/jpeg_tables_dev.h: $(CSRC)/gen_jpeg_tables.py
	python3 $< dev > $@

$(B)/%.o: $(CSRC)/%.hip $(HDRS)
	@mkdir -p $(B)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(B)/lz4r.o: HIPFLAGS += $(LZ4R_HIPFLAGS)
$(B)/lz4r_gpudec.o: HIPFLAGS += $(LZ4R_GPUDEC_HIPFLAGS)

$(B)/%.o: $(HOST)/%.c $(HDRS) $(HOST)/lzj_host.h
	@mkdir -p $(B)
	$(CC) $(CFLAGS_HOST) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^

chunk12: $(CHUNK12_LIB)

# A/B only, not part of `all`: jpegr_thumb.hip (self-contained) with the other
# form of its record read, for tools/jpeg_pack_bench.py --thumb --against
# (DESIGN 4.14).  The product reads through the LDS window; this one does not.
THUMB_ALT_LIB := $(B)/libjpegr_thumb_alt.so
thumb-alt: $(THUMB_ALT_LIB)

$(THUMB_ALT_LIB): $(CSRC)/jpegr_thumb.hip $(HDRS)
	@mkdir -p $(B)
	$(HIPCC) $(HIPFLAGS) -DJPRS_THUMB_WINDOW=0 -shared -o $@ $<

$(CHUNK12_LIB): $(CSRC)/lz4r.hip $(HDRS)
	@mkdir -p $(B)
	$(HIPCC) $(CHUNK12_HIPFLAGS) -shared -o $@ $<

# executables link the objects statically (no liblz4jpeg.so lookup at run time)
# how JPEG_dec and JPEG_sel open a .jpr file: the executables' alone, not the library's
JPR_FILE_OBJS := $(B)/jpr_file.o $(B)/read_file.o
$(BIN)/LZ4_seq: $(B)/lz4_seq.o $(OBJS)
	@mkdir -p $(BIN)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^

$(BIN)/LZ4_frame: $(B)/lz4_frame.o $(B)/read_file.o $(OBJS)
	@mkdir -p $(BIN)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^

$(BIN)/JPEG_seq: $(B)/jpeg_seq.o $(B)/png_io.o $(OBJS)
	@mkdir -p $(BIN)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^ -lz

$(BIN)/JPEG_dec: $(B)/jpeg_dec.o $(B)/png_io.o $(JPR_FILE_OBJS) $(OBJS)
	@mkdir -p $(BIN)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^ -lz

$(BIN)/JPEG_sel: $(B)/jpeg_sel.o $(JPR_FILE_OBJS) $(OBJS)
	@mkdir -p $(BIN)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^

# the parallel drivers' executables (Experiment/*_parallel_experiment.c)
$(B)/lz4_par.o: $(HOST)/lz4_seq.c $(HDRS)
	@mkdir -p $(B)
	$(CC) $(CFLAGS_HOST) -DLZ4_PAR -c $< -o $@

$(BIN)/LZ4_par: $(B)/lz4_par.o $(OBJS)
	@mkdir -p $(BIN)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^

$(BIN)/JPEG_par: $(BIN)/JPEG_seq
	cp $< $@

$(BIN)/%.exe: $(BIN)/%
	cp $< $@

oracle:
	$(MAKE) -C oracle

# ASan + UBSan build of the host C (no HIP) and the oracle restatements,
# driven by tests/sanitize/sanitize_main.c; tests/test_sanitize.py
SAN_SRC := tests/sanitize/sanitize_main.c tests/sanitize/cpu_matches.c $(HOST)/lz4r_decode.c \
           $(HOST)/png_io.c $(HOST)/read_file.c $(HOST)/synth.c $(HOST)/compat_lz4.c \
           oracle/lz4_oracle.c oracle/jpeg_oracle.c oracle/jpeg_entropy_oracle.c
sanitize: build/sanitize_main

SAN_FLAGS := -O1 -g -ffp-contract=off -fno-omit-frame-pointer \
             -fsanitize=address,undefined -fno-sanitize-recover=all

# sanitize_main.c's C++ siblings, whichever the tests directory holds
# (bare_layout.cpp: the decoder's scratch layout; csrc/lz4r_dec_layout.h is
# plain host C++), each compiled to an object of its own and linked in
# (frame_dev_main.cpp is a program of its own: sanitize-frame-dev below)
SAN_CXX_OBJ := $(patsubst tests/sanitize/%.cpp,build/san_%.o,\
                 $(filter-out tests/sanitize/frame_dev_main.cpp,$(wildcard tests/sanitize/*.cpp)))

build/san_%.o: tests/sanitize/%.cpp $(CSRC)/lz4r_dec_layout.h include/lz4r.h
	@mkdir -p build
	$(CXX) $(SAN_FLAGS) -std=c++17 -Wall -c $< -o $@

build/sanitize_main: $(SAN_SRC) $(SAN_CXX_OBJ) include/lz4r.h include/lz4jpeg_synth.h \
                     include/lz4jpeg_compat.h $(HOST)/lzj_host.h
	@mkdir -p build
	$(CC) $(SAN_FLAGS) -std=gnu11 -o $@ $(SAN_SRC) $(SAN_CXX_OBJ) -lz -lm -lpthread

# ASan + UBSan build of the standard-frame decoder alone (host/lz4f_decode.c),
# driven by tests/sanitize/frame_main.c; tests/test_sanitize_frame.py
sanitize-frame: build/sanitize_frame
	./build/sanitize_frame

build/sanitize_frame: tests/sanitize/frame_main.c $(HOST)/lz4f_decode.c $(HOST)/lz4f_xxh32.h include/lz4r.h
	@mkdir -p build
	$(CC) $(SAN_FLAGS) -std=gnu11 -Wall -o $@ tests/sanitize/frame_main.c $(HOST)/lz4f_decode.c

# ASan + UBSan build of what the GPU frame decoder's kernels parse with
# (csrc/lz4f_parse.h, compiled for the host) against host/lz4f_decode.c,
# driven by tests/sanitize/frame_dev_main.cpp; tests/test_sanitize_frame_dev.py
sanitize-frame-dev: build/sanitize_frame_dev
	./build/sanitize_frame_dev

build/san_lz4f_decode.o: $(HOST)/lz4f_decode.c $(HOST)/lz4f_xxh32.h include/lz4r.h
	@mkdir -p build
	$(CC) $(SAN_FLAGS) -std=gnu11 -Wall -c $< -o $@

build/sanitize_frame_dev: tests/sanitize/frame_dev_main.cpp build/san_lz4f_decode.o \
                          $(CSRC)/lz4f_parse.h $(HOST)/lz4f_xxh32.h include/lz4r.h
	@mkdir -p build
	$(CXX) $(SAN_FLAGS) -std=c++17 -Wall -o $@ tests/sanitize/frame_dev_main.cpp build/san_lz4f_decode.o

# micro-benchmarks: SIMD issue rates (tools/issue.sh) and LDS access costs
tools: tools/ab/valu_rate tools/ab/lds_rate

tools/ab/valu_rate: tools/valu_rate.hip
	@mkdir -p tools/ab
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<

tools/ab/lds_rate: tools/lds_rate.hip
	@mkdir -p tools/ab
	$(HIPCC) --offload-arch=$(ARCH) -O3 -Wno-unused-result -o $@ $<

clean:
	rm -rf $(B) $(BIN) $(LIB) build
	$(MAKE) -C oracle clean

.PHONY: all lib bin oracle tools chunk12 thumb-alt sanitize sanitize-frame sanitize-frame-dev clean

# `make -s print-HIPFLAGS`: a variable's value (tests/test_isa.py builds with the product flags)
print-%:
	@echo $($*)
