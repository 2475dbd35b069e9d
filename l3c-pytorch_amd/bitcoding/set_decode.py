"""SetDecoder -- `Bitcoding.decode_many`: a set of `.l3c` files of differently sized images, decoded on lanes (a stream pair per batch of
equally sized images) and in ragged groups (every predicted scale of many images in lock step).  It owns what only the set decode needs:
its knobs, the lane stream pairs, the stream pair of the ragged phases and the stream the ragged buffers are allocated on.  One scale record
of one batch is decoded by the Bitcoding it serves (the record checks, get_P, the coarsest scale); the chunk plans of the RGB scale are
Bitcoding's too (ragged_rgb_chunk_plan, banded_rgb_chunks: functions of its RGB_PROBE / RGB_CHUNKS)."""
import numpy as np
import torch

from .. import ops
from . import container, upload


class _Entry(object):
    """One entry of a ragged group -- a batch of B equally sized images -- as it moves through the group's phases."""
    __slots__ = ('index', 'files', 'parsed', 'records', 'B', 'lane', 'F', 'streams', 'sym', 'hw')

    def __init__(self, index, files, parsed, records, lane):
        self.index, self.files = index, files          # position in decode_many's `batches`; the entry's `.l3c` byte strings
        self.parsed, self.records = parsed, records    # upload-ready framing (container.ParsedFraming); the format's own scale headers
        self.B, self.lane = len(files), lane           # images; (main stream, side stream) of the entry's lane
        self.F = None                                  # the network's feature carry of get_P, scale to scale
        self.streams = None                            # upload._DeviceStreams: the files' streams on the device
        self.sym, self.hw = None, None                 # the symbols (B, C, H, W) and the (H, W) of the scale decoded last


class SetDecoder(object):
    N_DECODE_LANES = 8               # lanes when every batch is small (fewer than 64 images: latency-bound chains); large batches run one after the other
    RAGGED_GROUP = 512               # at most this many images are decoded together as one ragged group ...
    RAGGED_GROUP_PIXELS = 128 << 20  # ... and at most this many pixels (P of the RGB scale is 480 bytes per pixel: 64 GB; its tables 8 GB)
    ENTRY_LIMIT = ops.ENTRIES_MAX    # entries (images, bands) per ragged library call; a larger group goes through in slices

    def __init__(self, bitcoding):
        """bitcoding: the Bitcoding whose model, constants and single-batch decoder this set decoder uses.  The knobs above are class
        attributes; an instance may override them."""
        self.bc = bitcoding
        # the streams of the set decode, created by _own_streams
        self._lane_streams, self._lane_key = None, None
        self._rgb_streams = None
        self._alloc_stream = None
        # sealed=True: {(entry, file): CRC-32 the device computed of that file's decoded frame} of the last call (lane and ragged forms)
        self.frame_crcs = {}

    def _own_streams(self, n, chain_cus, ragged):
        """Creates what is missing of: `n` lane pairs (main stream, side stream); for the ragged form the stream pair of the ragged phases and
        the stream the ragged buffers are allocated on.  chain_cus > 0: every lane's side stream -- the latency-bound range-decoder chains --
        is confined to `chain_cus` compute units (the same number of every XCD, helpers/runtime.balanced_cu_sets) and every main stream --
        convolutions, table kernels -- to the others, so that a lane's MFMA wavefronts never take the registers or the issue slots of
        another lane's chains."""
        key = (n, chain_cus)
        if self._lane_key != key:
            from .. import _lib
            if chain_cus:
                from ..helpers import runtime
                _, n_cu, _ = _lib.device_info()
                chains, rest = runtime.balanced_cu_sets(n_cu, chain_cus)
                self._lane_streams = [(_lib.cu_mask_stream(rest), _lib.cu_mask_stream(chains)) for _ in range(n)]
            else:
                self._lane_streams = [(torch.cuda.Stream(), torch.cuda.Stream()) for _ in range(n)]
            self._lane_key = key
        if ragged and self._rgb_streams is None:
            self._rgb_streams = (torch.cuda.Stream(), torch.cuda.Stream())
            self._alloc_stream = torch.cuda.Stream()

    def decode_many(self, batches, on_batch, lanes, chain_cus, out_dtype, ragged, banded, sealed=False):
        """Bitcoding.decode_many (the arguments and the result are described there)."""
        seals, self.frame_crcs = None, {}
        if sealed:
            sealed_files = batches
            batches, seals = self._split_seals(sealed_files)
        elif any(container.is_sealed(f) for files in batches for f in files):
            raise ValueError('decode_many does not read sealed .l3c files unless it is told to (sealed=True verifies them): '
                             'container.split_seal gives the body and the seal to check, or decode_batch / decode verify them')
        fmt = [any(container.is_banded(f) for f in files) for files in batches]
        if any(fmt) and not banded:
            raise ValueError('decode_many reads legacy .l3c files only: a banded file (L3CB format) goes through decode_batch / decode')
        n = self.N_DECODE_LANES if lanes is None else int(lanes)
        if lanes is None and max(len(f) for f in batches) >= 64:
            n = 1
        result = [None] * len(batches)
        if n <= 1 or len(batches) <= 1:
            for i, files in enumerate(sealed_files if sealed else batches):
                try:
                    pixels, padding = self.bc.decode_batch(files, out_dtype)        # verifies the sealed files of the batch itself
                except container.SealError as e:
                    raise container.SealError(e.reason, (i, e.index), 'entry {}: {}'.format(i, e), [(i, k) for k in e.failed])
                if on_batch is not None:
                    on_batch(i, pixels, padding)
                else:
                    result[i] = (pixels, padding)
            return result
        self.bc.blueprint.net._prepare()               # pack the weights before forking streams
        outer = torch.cuda.current_stream()
        start = torch.cuda.Event()
        start.record(outer)
        use_ragged = (ragged is None or ragged) and all(len(f) < 64 for f in batches)
        self._own_streams(n, chain_cus, use_ragged)
        for main, _ in self._lane_streams:
            main.wait_event(start)
        done = []
        words = []                                     # sealed: (CRC words on the device, [(entry, file)] they belong to) per batch or group

        def finish(i, pixels, padding, stream):
            if on_batch is not None:
                on_batch(i, pixels, padding)
            else:
                pixels.record_stream(outer)
                result[i] = (pixels, padding)

        if not use_ragged:
            for i, files in enumerate(batches):
                main, side = self._lane_streams[i % n]
                check = seals is not None and any(s is not None for s in seals[i])
                with torch.cuda.stream(main):
                    pixels, padding = self.bc._decode_batch(files, torch.uint8 if check else out_dtype, side)
                    if check:
                        B = pixels.shape[0]
                        words.append((ops.u8_crc32(pixels.view(-1), B, pixels.numel() // B), [(i, k) for k in range(B)]))
                        pixels = pixels.to(out_dtype)
                    finish(i, pixels, padding, main)
                    done.append(main.record_event())
        else:
            rgb_main = self._rgb_streams[0]
            rgb_main.wait_event(start)
            for group, b in self._plan_groups(batches, fmt):
                check = seals is not None and any(s is not None for i, _ in group for s in seals[i])
                self.decode_group(group, out_dtype, finish, banded=b, words=words if check else None)
            done.append(rgb_main.record_event())
        for ev in done:
            outer.wait_event(ev)
        if words:
            self._check_words(words, seals, outer)
        return result

    def _split_seals(self, batches):
        """sealed=True, before anything is enqueued: every file split into body and seal (container.split_seal: a view, not a copy), every
        seal's generation and model id checked (container.check_seals over all files of the call; SealError with index (entry, file)).
        -> (the bodies, the seals) in the shape of `batches`."""
        split = [[container.split_seal(f, view=True) for f in files] for files in batches]
        where = [(i, k) for i, files in enumerate(batches) for k in range(len(files))]
        try:
            container.check_seals([s for fs in split for _, s in fs], self.bc.generation(), self.bc.model_id)
        except container.SealError as e:
            raise container.SealError(e.reason, where[e.index], 'entry {} file {}: {}'.format(*where[e.index], e))
        return [[b for b, _ in fs] for fs in split], [[s for _, s in fs] for fs in split]

    def _check_words(self, words, seals, outer):
        """sealed=True, at the end of the call: ONE D2H of every CRC word the lanes and groups left on the device (`outer` has waited for all
        of them), compared with the seals; SealError('pixels') naming the first failing file in call order, .failed listing all."""
        for t, _ in words:
            t.record_stream(outer)
        host = torch.cat([t for t, _ in words]).cpu().numpy().view(np.uint32).tolist()
        self.frame_crcs = dict(zip([key for _, keys in words for key in keys], host))
        failed = sorted(key for key, w in self.frame_crcs.items() if seals[key[0]][key[1]] is not None and seals[key[0]][key[1]].frame_crc != w)
        if failed:
            i, k = failed[0]
            raise container.SealError('pixels', (i, k), 'entry {} file {} decoded to pixels whose CRC-32 {:08x} is not the sealed {:08x}: damaged '
                                      'payload, or not the checkpoint that wrote it ({} of the call\'s files failed)'.format(
                                          i, k, self.frame_crcs[i, k], seals[i][k].frame_crc, len(failed)), failed)

    def _plan_groups(self, batches, fmt):
        """The ragged groups of a set, in decoding order -> (group: [(index, files)], banded) each; fmt[i]: entry i holds banded files.
        Groups of (nearly) EQUAL pixel counts below the budget: [measured, profiles/r06_set_decode_group_budget.log, 500 images = 312 MPix]
        groups of 48 / 96 / 160 MPix: 69 / 95 / 32 MPix/s (peak 55 / 96 / 157 GB: two consecutive groups' buffers then no longer fit the
        allocator's caches and every phase pays hipFree + hipMalloc)."""
        pix = []
        for files, b in zip(batches, fmt):
            H, W = container.padded_shape(files[0]) if b else container.parse_containers(files[:1]).scales[-1][1:]
            pix.append(len(files) * H * W)
        for b in (False, True):        # format-pure groups: the legacy entries, then the banded ones
            idx = [i for i in range(len(batches)) if fmt[i] == b]
            if not idx:
                continue
            n_groups = max(1, -(-sum(pix[i] for i in idx) // self.RAGGED_GROUP_PIXELS))
            target = sum(pix[i] for i in idx) / float(n_groups)
            group, n_img, n_pix = [], 0, 0
            for i in idx:
                group.append((i, batches[i]))
                n_img += len(batches[i])
                n_pix += pix[i]
                if n_img >= self.RAGGED_GROUP or n_pix >= target or i == idx[-1]:
                    yield group, b
                    group, n_img, n_pix = [], 0, 0

    # ---- one ragged group ---------------------------------------------------------------------------------------------------------

    def decode_group(self, group, out_dtype, finish, banded=False, words=None):
        """One group of decode_many's ragged form, in PHASES over all its entries (batches of different shapes):
            lanes:   upload, the coarsest scale (uniform prior), P of the next scale (get_P per shape)      -- small launches, a lane per entry
            ragged:  that scale's symbols of ALL images in lock step (bottleneck scale: one table launch + one decoder launch for every
                     image and channel; RGB scale: the chunk pipeline of l3c_decode_rgb_ragged), on the stream pair of the ragged phases
            lanes:   P of the next finer scale ...                                                          -- and so on down to scale 0
        An image's serial chains -- 12 ms at scale 1, 60-70 ms at scale 0 for 768x512 -- are thereby paid once per GROUP instead of once
        per image; what is left per image are the decoder-side convolutions of its shape.
        banded: the group's files are BANDED (an entry's files share the band length of every scale).  The phases are the same; a ragged
        phase then runs over every band of every image as an entry of its own -- pixels [j L, j L + len_j) of its image -- and the chains
        paid per group are a band long.  A legacy group is the same with one entry per image.
        words (decode_many's sealed=True, a group with sealed files): behind the last scale the group's symbols become pixels in ONE launch
        (ops.sym_to_u8 over the whole ragged buffer) and ONE ops.u8_crc32_spans hashes every image's frame -- image b of entry g is bytes
        [3 pixbase[g] + b 3 H W, + 3 H W) -- on the stream of the ragged phases; (the words on the device, their (entry, file)) is appended
        to `words`, nothing waits for them here.  uint8 results are then views of that pixel buffer."""
        st, n_pred = self._parse_group(group, banded)
        plan = list(self.bc.iter_scale_dmll(n_pred))          # record k -> (scale, dmll, uniform), coarse -> fine
        self._decode_coarsest(st, plan[0], banded)
        keep = []
        for k in range(1, n_pred + 1):
            scale, dmll, _ = plan[k]
            P_rag, sym_rag, pixbase, hws = self._predict_scale(st, k, scale, dmll, plan[k - 1][1], n_pred)
            base_t, offs, lens = self._group_stream_table(st, k)
            done, hold = self._decode_symbols(st, k, dmll, P_rag, sym_rag, pixbase, hws, base_t, offs, lens, k == n_pred, banded)
            keep.append(hold)
            self._hand_back(st, k, sym_rag, pixbase, done)
            del P_rag          # (its block goes back to the allocator as soon as the streams that touched it have passed this point: a group's three P buffers never pile up)
        rgb_main = self._rgb_streams[0]
        with torch.cuda.stream(rgb_main):
            if words is not None:
                pix = ops.sym_to_u8(sym_rag)
                offs, lens, keys = [], [], []
                for g, e in enumerate(st):
                    n = 3 * e.hw[0] * e.hw[1]
                    offs += [3 * pixbase[g] + b * n for b in range(e.B)]
                    lens += [n] * e.B
                    keys += [(e.index, b) for b in range(e.B)]
                words.append((ops.u8_crc32_spans(pix, offs, lens), keys))
            for g, e in enumerate(st):
                if words is not None and out_dtype == torch.uint8:
                    H, W = e.hw
                    out = pix[3 * pixbase[g]:3 * (pixbase[g] + e.B * H * W)].view(e.B, 3, H, W)
                else:
                    out = e.sym.to(out_dtype)
                finish(e.index, out, e.parsed.padding, rgb_main)
        del keep

    def _parse_group(self, group, banded):
        """Phase 1: every entry's framing, parsed and checked against the model -> (entries, predicted scales of the set's files)."""
        n = len(self._lane_streams)
        st, n_preds = [], set()
        for i, files in group:
            if banded:
                records, parsed = container.parse_set_entry(files)
            else:
                parsed = container.parse_containers(files)
                records = parsed.scales
            n_preds.add(self.bc._n_predicted(len(records)))
            self.bc._check_coarsest(records[0], banded, int(parsed.nbytes[0].max()))
            st.append(_Entry(i, files, parsed, records, self._lane_streams[i % n]))
        if len(n_preds) != 1:
            raise ValueError('decode_many: the files of a set must come from one model (different numbers of scale records)')
        return st, n_preds.pop()

    def _decode_coarsest(self, st, plan0, banded):
        """Phase 2: upload and the coarsest scale (uniform prior), one launch per entry on its lane."""
        scale, dmll, uniform = plan0
        assert uniform
        symbols = self.bc._scale_symbols_of(banded)
        for e in st:
            with torch.cuda.stream(e.lane[0]):
                e.streams = upload._upload_streams(e.files, e.parsed)
                e.sym, _ = symbols(e.streams, 0, e.records[0], dmll, True, None, e.B, None)
                e.hw = tuple(e.records[0][1:3])

    def _ragged_buffers(self, n_floats, n_sym, mains):
        """P and (zeroed) symbol buffer of one scale of the group -> (P_rag, sym_rag, event behind the zero fill)."""
        # from a stream that runs nothing but the zero fill: allocated under rgb_main they would be ordered behind the previous group's whole
        # last phase (the allocator reuses a stream's blocks in stream order) and every lane of this group would wait for it
        with torch.cuda.stream(self._alloc_stream):
            P_rag = torch.empty(n_floats, dtype=torch.float32, device='cuda')
            sym_rag = torch.zeros(n_sym, dtype=torch.int16, device='cuda')
            ev = self._alloc_stream.record_event()
        for t in (P_rag, sym_rag):
            for s_ in mains + list(self._rgb_streams):
                t.record_stream(s_)
        return P_rag, sym_rag, ev

    def _predict_scale(self, st, k, scale, dmll, prev, n_pred):
        """Phase 3: record k's headers against the network, then P of that scale on the lanes (get_P per entry, fed the symbols of the
        scale above, coded with `prev`), written into the group's ragged buffer.  -> (P_rag, sym_rag, first pixel of every entry in them,
        pixels of every image); the stream of the ragged phases waits for every lane."""
        rgb_main = self._rgb_streams[0]
        hws, pixbase, p = [], [], 0
        for e in st:
            Cs, H, W = e.records[k][:3]
            Kp = self.bc._check_header(scale, dmll, (Cs, H, W), e.hw)
            pixbase.append(p)
            p += e.B * H * W
            hws += [H * W] * e.B
            e.hw = (H, W)
        P_rag, sym_rag, alloc_ev = self._ragged_buffers(p * Kp, Cs * p, [m for m, _ in self._lane_streams])
        rgb_main.wait_event(alloc_ev)
        for g, e in enumerate(st):
            main = e.lane[0]
            main.wait_event(alloc_ev)
            with torch.cuda.stream(main):
                H, W = e.hw
                P, e.F = self.bc._get_P(scale, n_pred, self.bc._next_input(e.sym, prev), e.F, (e.B, H, W, Kp))
                P_rag[pixbase[g] * Kp:(pixbase[g] + e.B * H * W) * Kp].view(e.B, H, W, Kp).copy_(P)
                rgb_main.wait_event(main.record_event())
        return P_rag, sym_rag, pixbase, hws

    @staticmethod
    def _group_stream_table(st, k):
        """Phase 4: one stream table of record k for the whole group, on the host: CHANNEL-major over all entries -- per channel the streams of
        the group in the order (entry, image, band), a legacy image being one band.  Every entry keeps its own stream buffer, addressed from
        the lowest one.  -> (that buffer, offsets int64 (C, S), lengths int32 (C, S))."""
        base_t = min((e.streams.buf for e in st), key=lambda t: t.data_ptr())
        Cs = st[0].records[k][0]
        o_all, l_all = [], []
        for e in st:
            o, l = e.streams.scale_host_channel_image_band(k, Cs, e.B)
            o_all.append(o + (e.streams.buf.data_ptr() - base_t.data_ptr()))
            l_all.append(l)
        return base_t, np.concatenate(o_all, axis=1).astype(np.int64), np.concatenate(l_all, axis=1).astype(np.int32)

    @staticmethod
    def _entry_table(st, k, pixbase, banded):
        """(pixbase, hw, pix0, length) of the group's ragged entries of record k, in the stream table's order: every band of every image of
        a banded group, every image of a legacy one."""
        rows = []
        for g, e in enumerate(st):
            H, W = e.records[k][1:3]
            rows.append(container.band_entry_table(e.B, H * W, e.records[k][3], pixbase[g]) if banded else
                        container.image_entry_table([H * W] * e.B, pixbase[g]))
        return [np.concatenate(a) for a in zip(*rows)]

    def _decode_symbols(self, st, k, dmll, P_rag, sym_rag, pixbase, hws, base_t, offs, lens, last, banded):
        """Phase 5: record k's symbols of the whole group, on the stream pair of the ragged phases.  Bottleneck scales: ragged table and decoder
        launches over the entries (_decode_z_entries).  RGB scales: the chunk pipeline over all entries in lock step -- of legacy files
        l3c_decode_rgb_ragged, an image an entry; of banded files l3c_decode_rgb_entries, the chunk count bounded by the legacy group
        decode's workspace for the same images (banded_rgb_chunks), more than ENTRY_LIMIT entries in slices.
        -> (event behind the symbols, tensors to keep alive)."""
        bc, K = self.bc, self.bc.blueprint.net.config_ms.prob.K
        rgb_main, rgb_side = self._rgb_streams
        targets = bc._targets(dmll)
        with torch.cuda.stream(rgb_main):
            for e in st:
                e.streams.buf.record_stream(rgb_main)
                e.streams.buf.record_stream(rgb_side)
                if last:
                    e.streams.finish()       # the bulk of the files (the last record) crosses PCIe here, behind the convolutions just enqueued
            if not dmll.rgb_scale:
                hold = self._decode_z_entries(P_rag, targets, sym_rag, base_t, offs, lens, self._entry_table(st, k, pixbase, banded), K)
            elif banded:
                base, hw, pix0, length = self._entry_table(st, k, pixbase, banded)
                lag, mode, side = bc._rgb_schedule(hw.shape[0], rgb_side)
                chunks, _ = bc.banded_rgb_chunks(hws, length, bc.rgb_window, bc._rgb_schedule(len(hws), rgb_side)[0], lag)
                hold = ops.decode_rgb_entries(P_rag, targets, sym_rag, base_t, offs, lens, base, hw, pix0, length, chunks, K, lag, mode, side,
                                              limit=self.ENTRY_LIMIT)
            else:
                offs_d = ops.upload_small(offs.reshape(-1))
                lens_d = ops.upload_small(lens.reshape(-1))
                pix0, npix = bc.ragged_rgb_chunk_plan(hws, bc.rgb_window)
                hold = (offs_d, lens_d, ops.decode_rgb_ragged(P_rag, targets, sym_rag, base_t, offs_d, lens_d, hws, pix0, npix, K,
                                                              *bc._rgb_schedule(len(hws), rgb_side)))
            return rgb_main.record_event(), (sym_rag, hold)

    def _decode_z_entries(self, P_rag, targets, sym_rag, buf, offs, lens, table, K):
        """A bottleneck scale of the group on the current stream: one ragged table launch and one ragged decoder launch over all entries
        (ops.decode_z_entries), more than ENTRY_LIMIT entries in slices.  -> tensors to keep alive."""
        base, hw, pix0, length = table
        C, total = offs.shape[0], sym_rag.numel() // offs.shape[0]
        # Every slice's call allocates its C tables for the pixels of the WHOLE group (ops.decode_z_entries addresses a table row by its
        # pixel in the group), and all of them live until the group is done: the bottleneck tables are paid once per SLICE.  A group has at
        # most RAGGED_GROUP images of at most K bands each, so K = 64 never slices (32 768 bands) and K = 256 slices in three at the most;
        # tables sized per slice would need slice-relative table offsets in ops.decode_z_entries.
        keep = []
        for a, b in ops.entry_slices(hw.shape[0], self.ENTRY_LIMIT):
            offs_d = ops.upload_small(np.ascontiguousarray(offs[:, a:b]).reshape(-1))
            lens_d = ops.upload_small(np.ascontiguousarray(lens[:, a:b]).reshape(-1))
            keep.append((offs_d, lens_d, ops.decode_z_entries(P_rag, targets, sym_rag, buf, offs_d, lens_d, base[a:b], hw[a:b], pix0[a:b],
                                                              length[a:b], total, C, K)))
        return keep

    @staticmethod
    def _hand_back(st, k, sym_rag, pixbase, done):
        """Phase 6: every entry's view of the group's symbols; its lane goes on behind the ragged phase (`done`)."""
        Cs = st[0].records[k][0]
        for g, e in enumerate(st):
            H, W = e.hw
            a = Cs * pixbase[g]
            e.sym = sym_rag[a:a + Cs * e.B * H * W].view(e.B, Cs, H, W)
            e.lane[0].wait_event(done)
