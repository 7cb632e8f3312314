"""Dataset loaders for --datadir: the reference's list files, frame indices, file names and WAV windows (utils/video_dataset.py),
handed over in the forms the input kernels take.

    python -m adamml_amd.train ... --dense_sampling --datadir RGB_DIR SOUND_DIR --loader_factory adamml_amd.data:loaders

`loaders(args, rank, world, device)` builds a `MultiVideoDataSet` for training and one for validation and wraps each in a
DataLoader.  A worker only reads files: per video it draws the frame indices (numpy's global RNG, as the reference does), reads the
frames' JPEG files as bytes, draws each visual modality's crop / scale / flip (`video.Augmentor.sample`, in --modality order) and
cuts the sound windows out of the WAV track.  `Collate` packs a batch as `video.EncodedFrames` per visual modality (decoded,
augmented, differenced and normalised on the GPU) and one `audio.Waveforms` for sound (log-spectrogram on the GPU); a batch holding a
JPEG file the GPU decoder does not take is decoded with Pillow into a `video.Frames` instead.  AdaMML.forward takes all three."""
import io
import os
import struct

import numpy as np
import torch

from . import audio, jpeg, video

__all__ = ['Collate', 'DATASETS', 'Loader', 'MultiVideoDataSet', 'VideoDataSet', 'VideoRecord', 'loaders', 'random_clip', 'read_wav',
           'sample_train_clip', 'sample_val_test_clip']

# per dataset (utils/dataset_config.py:18-28, the one entry the reference ships): list files, separator, frame template, filter_video
DATASETS = {'kinetics-sounds': dict(train_list='train.txt', val_list='val.txt', separator=';', image_tmpl='{:05d}.jpg', filter_video=0)}
CONSECUTIVE = 5          # frames per index of the flow and rgbdiff modalities
PCM_SUBFORMAT = b'\x01\x00\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'

pillow_fallbacks = 0     # batches of a visual modality that were decoded with Pillow (counted in the process that collates)


# ---------------------------------------------------------------------------------------------- frame indices (0-based inside, 1-based out)
def random_clip(video_frames, sampling_rate, frames_per_clip, fixed_offset=False, start_frame_idx=0, end_frame_idx=None):
    """frames_per_clip indices (from zero), sampling_rate apart and wrapped at video_frames.  The clip starts at a random offset in
    [start_frame_idx, end_frame_idx) -- end_frame_idx defaults to the last start that fits -- at the centred offset with fixed_offset,
    and at 0 when nothing fits (video_dataset.py:7-29).  One np.random.randint draw, or none."""
    span = sampling_rate * frames_per_clip
    highest = video_frames - span if end_frame_idx is None else end_frame_idx
    if highest <= 0:
        offset = 0
    elif fixed_offset:
        offset = (video_frames - span) // 2
    else:
        offset = int(np.random.randint(start_frame_idx, highest, 1)[0])
    return [int(offset + i * sampling_rate) % video_frames for i in range(frames_per_clip)]


def _uniform_draw(max_frame_idx, num_frames, sample_freq, seed=None):
    """One uniform clip (unsorted): sample_freq offsets shared by every one of num_frames equal groups when the groups are long
    enough, else num_frames * sample_freq random frames (with repeats only if the video is too short).  `seed` re-seeds numpy's
    global RNG before the two fallback draws (the validation quirk of video_dataset.py:222-229)."""
    total = num_frames * sample_freq
    per_group = max_frame_idx // num_frames
    if per_group >= sample_freq:
        base = np.repeat(np.arange(0, num_frames) * per_group, repeats=sample_freq)
        offsets = np.random.choice(per_group, sample_freq, replace=False)
        return base + np.tile(offsets, num_frames)
    if seed is not None:
        np.random.seed(seed)
    if max_frame_idx < total:
        return np.random.choice(max_frame_idx, total)
    return np.random.choice(max_frame_idx, total, replace=False)


def sample_train_clip(video_length, num_consecutive_frames, num_frames, sample_freq, dense_sampling, num_clips=1):
    """Training indices, 1-based (video_dataset.py:135-170).  Dense: num_clips clips of num_frames frames sample_freq apart, clip i
    starting in the i-th of num_clips equal stretches of the possible starts (anywhere when the stretches are empty, or for one clip).
    Uniform: one sorted clip of num_frames * sample_freq frames -- num_clips is ignored."""
    max_frame_idx = max(1, video_length - num_consecutive_frames + 1)
    if not dense_sampling:
        return np.sort(_uniform_draw(max_frame_idx, num_frames, sample_freq)) + 1
    idx = np.zeros((num_clips, num_frames), dtype=int)
    stretch = 0 if num_clips == 1 else (max_frame_idx - sample_freq * num_frames) // num_clips
    for i in range(num_clips):
        if stretch <= 0:
            idx[i] = random_clip(max_frame_idx, sample_freq, num_frames)
        else:
            idx[i] = random_clip(max_frame_idx, sample_freq, num_frames, False, i * stretch, (i + 1) * stretch)
    return idx.flatten() + 1


def sample_val_test_clip(video_length, num_consecutive_frames, num_frames, sample_freq, dense_sampling, fixed_offset, num_clips):
    """Validation / test indices, 1-based (video_dataset.py:173-233).  Dense + fixed_offset: num_clips clips whose starts are spread
    evenly over the possible starts; dense without: num_clips random clips.  Uniform + fixed_offset: per clip the centres of num_frames
    equal ticks shifted by the clip's offset in -num_clips // 2 + 1 .. num_clips // 2 (clamped to half a tick), or, for a video no
    longer than num_frames, num_frames random frames after np.random.seed(clip number).  Uniform without: num_clips uniform clips as in
    training, whose fallback draws re-seed numpy with the clip number."""
    max_frame_idx = max(1, video_length - num_consecutive_frames + 1)
    out = []
    if dense_sampling and fixed_offset:
        last_start = max(1, 1 + max_frame_idx - sample_freq * num_frames) - 1
        for start in np.linspace(0, last_start, num=num_clips, dtype=int).tolist():
            out += [(i * sample_freq + start) % max_frame_idx for i in range(num_frames)]
    elif dense_sampling:
        for _ in range(num_clips):
            out += random_clip(max_frame_idx, sample_freq, num_frames)
    elif fixed_offset:
        first = -num_clips // 2 + 1
        for shift in range(first, num_clips // 2 + 1):
            if max_frame_idx > num_frames:
                tick = max_frame_idx / float(num_frames)
                s = shift
                if s >= tick / 2.0:
                    s = tick / 2.0 - 1e-4
                elif s < -tick / 2.0:
                    s = -tick / 2.0
                clip = np.array([int(tick / 2.0 + s + tick * x) for x in range(num_frames)])
            else:
                np.random.seed(shift - first)
                clip = np.random.choice(max_frame_idx, num_frames)
            out += np.sort(clip).tolist()
    else:
        for i in range(num_clips):
            out += np.sort(_uniform_draw(max_frame_idx, num_frames, sample_freq, seed=i)).tolist()
    return np.asarray(out) + 1


# ---------------------------------------------------------------------------------------------- WAV tracks
def read_wav(path):
    """The track of a 16-bit PCM RIFF/WAVE file as librosa.load(path, sr=None, mono=True) returns it for the files
    tools/extract_audio.py writes (pcm_s16le): int16 / 32768 as float32, the float32 mean over the channels of a multi-channel file.
    The file's own rate is not looked at (the reference drops it too).  Format 1 and WAVE_FORMAT_EXTENSIBLE with the PCM subformat."""
    with open(path, 'rb') as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b'RIFF' or raw[8:12] != b'WAVE':
        raise ValueError("read_wav: %s is not a RIFF/WAVE file" % path)
    at, fmt, data = 12, None, None
    while at + 8 <= len(raw) and data is None:
        tag, size = raw[at:at + 4], struct.unpack_from('<I', raw, at + 4)[0]
        body = raw[at + 8:at + 8 + size]                # a streamed file may state more than it holds: the slice stops at the end
        if tag == b'fmt ':
            if len(body) < 16:
                raise ValueError("read_wav: %s has a truncated fmt chunk" % path)
            fmt = struct.unpack_from('<HHIIHH', body, 0)
            if fmt[0] == 0xFFFE:
                if len(body) < 40:
                    raise ValueError("read_wav: %s has a truncated WAVE_FORMAT_EXTENSIBLE fmt chunk" % path)
                if body[24:40] != PCM_SUBFORMAT:
                    raise ValueError("read_wav: %s is WAVE_FORMAT_EXTENSIBLE with subformat %s, expected 16-bit PCM"
                                     % (path, body[24:40].hex()))
            elif fmt[0] != 1:
                raise ValueError("read_wav: %s has format %d, expected 16-bit PCM (format 1)" % (path, fmt[0]))
            if fmt[5] != 16:
                raise ValueError("read_wav: %s has format %d with %d bits per sample, expected 16-bit PCM" % (path, fmt[0], fmt[5]))
            if fmt[1] < 1:
                raise ValueError("read_wav: %s states %d channels" % (path, fmt[1]))
        elif tag == b'data':
            data = body
        at += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError("read_wav: %s has no %s chunk" % (path, 'fmt' if fmt is None else 'data'))
    ch = fmt[1]
    pcm = np.frombuffer(data, '<i2', count=len(data) // (2 * ch) * ch).reshape(-1, ch)
    x = pcm.astype(np.float32) / np.float32(32768.0)
    return x[:, 0].copy() if ch == 1 else np.mean(x.T, axis=0)


# ---------------------------------------------------------------------------------------------- records and datasets
class VideoRecord(object):
    """One list line: folder (or WAV file) below the root, first and last frame, label(s); `line` is its number in the list."""

    def __init__(self, path, start_frame, end_frame, label, reverse=False, line=None):
        self.path = path
        self.video_id = os.path.basename(path)
        self.start_frame = start_frame
        self.end_frame = end_frame
        self.label = label
        self.reverse = reverse
        self.line = line

    @property
    def num_frames(self):
        return self.end_frame - self.start_frame + 1

    def __str__(self):
        return self.path


def _frame_size(blob, name):
    """(width, height) from a frame file's header."""
    try:
        inf = jpeg.parse(blob)
        return inf.width, inf.height
    except jpeg.Unsupported:
        from PIL import Image
        try:
            with Image.open(io.BytesIO(blob)) as im:
                return im.size
        except Exception as e:
            raise ValueError("cannot read the size of %s: %s" % (name, e)) from None


class VideoDataSet(torch.utils.data.Dataset):
    """One modality of a dataset (video_dataset.py:253-428): `root_path/list_file` lists `path<sep>start<sep>end<sep>label...` lines;
    rgb / rgbdiff frames are `root_path/path/image_tmpl.format(n)`, flow frames the same names with x_ / y_ in front, sound tracks
    `root_path/path`.  With dense_sampling num_groups is the number of frames of a clip and frames_per_group their spacing.
    `augmentor` is a `video.Augmentor` (visual modalities).  `get_data` returns file bytes, not images."""

    def __init__(self, root_path, list_file, num_groups=64, frames_per_group=1, num_clips=1, modality='rgb', dense_sampling=False,
                 fixed_offset=True, image_tmpl='{:05d}.jpg', augmentor=None, is_train=True, test_mode=False, separator=' ',
                 filter_video=0, num_classes=None, fps=29.97, audio_length=1.28, resampling_rate=24000, log=None):
        if modality not in ['flow', 'rgb', 'rgbdiff', 'sound']:
            raise ValueError("modality should be 'flow' or 'rgb' or 'rgbdiff' or 'sound'.")
        self.root_path = root_path
        self.list_file = os.path.join(root_path, list_file)
        self.num_groups = self.num_frames = num_groups
        self.frames_per_group = self.sample_freq = frames_per_group
        self.num_clips = num_clips
        self.fixed_offset = fixed_offset
        self.dense_sampling = dense_sampling
        self.modality = modality.lower()
        self.image_tmpl = image_tmpl
        self.augmentor = augmentor
        self.is_train = is_train
        self.test_mode = test_mode
        self.separator = separator
        self.filter_video = filter_video
        self.fps = fps
        self.audio_length = audio_length
        self.resampling_rate = resampling_rate
        self.num_consecutive_frames = CONSECUTIVE if self.modality in ('flow', 'rgbdiff') else 1
        self.log = log
        self.video_list, self.multi_label = self._parse_list()
        self.num_classes = num_classes

    def _parse_list(self):
        """Lines of [path, start_frame, end_frame, label, ...]; videos shorter than filter_video are dropped unless test_mode.
        The list is multi-label when its kept lines have more than 4 fields on average."""
        rows, total = [], 0
        with open(self.list_file) as f:
            for number, text in enumerate(f, 1):
                fields = text.strip().split(self.separator)
                if len(fields) < 3:
                    raise ValueError("%s, line %d: expected path%sstart%send[%slabel ...], got %r"
                                     % (self.list_file, number, self.separator, self.separator, self.separator, text.strip()))
                total += 1
                if self.test_mode or int(fields[2]) - int(fields[1]) + 1 >= self.filter_video:
                    rows.append((number, fields))
        if self.log is not None:
            self.log("The number of videos is {} (with more than {} frames) (original: {})".format(len(rows), self.filter_video, total))
        if not rows:
            raise ValueError("%s lists no video of at least %d frames" % (self.list_file, self.filter_video))
        multi_label = float(np.mean([len(fields) for _, fields in rows])) > 4.0
        records = []
        for number, fields in rows:
            if self.test_mode:
                label = -1
            else:
                label = [float(v) for v in fields[3:]]
                if not multi_label and len(label) == 1:
                    label = label[0]
            records.append(VideoRecord(fields[0], int(fields[1]), int(fields[2]), label, line=number))
        if self.modality == 'rgbdiff':                     # a difference needs the next frame
            for r in records:
                r.end_frame -= 1
        return records, multi_label

    def _sample_indices(self, record):
        return sample_train_clip(record.num_frames, self.num_consecutive_frames, self.num_frames, self.sample_freq, self.dense_sampling,
                                 self.num_clips)

    def _get_val_indices(self, record):
        return sample_val_test_clip(record.num_frames, self.num_consecutive_frames, self.num_frames, self.sample_freq, self.dense_sampling,
                                    self.fixed_offset, self.num_clips)

    def frame_numbers(self, record, seg_ind):
        """The num_consecutive_frames frame numbers of index seg_ind, clipped the reference's way (at num_frames, video_dataset.py:406)."""
        return [min(int(seg_ind) + record.start_frame - 1 + i, record.num_frames) for i in range(self.num_consecutive_frames)]

    def file_names(self, record, indices):
        """Paths below root_path of the files `indices` select, in the channel order the kernels stack them."""
        names = []
        for seg_ind in indices:
            numbers = self.frame_numbers(record, seg_ind)
            if self.modality == 'rgb':
                names += [self.image_tmpl.format(n) for n in numbers]
            elif self.modality == 'flow':
                for n in numbers:
                    names += ["x_" + self.image_tmpl.format(n), "y_" + self.image_tmpl.format(n)]
            else:
                if numbers != list(range(numbers[0], numbers[0] + len(numbers))):
                    raise ValueError("rgbdiff: video %s (%s, line %s): index %d of indices %s selects frames %s, clipped at the video's "
                                     "%d frames; their differences are not those of consecutive frames"
                                     % (record.path, self.list_file, record.line, int(seg_ind), [int(v) for v in indices], numbers,
                                        record.num_frames))
                names += [self.image_tmpl.format(n) for n in range(numbers[0], numbers[0] + len(numbers) + 1)]
        return [os.path.join(record.path, n) for n in names]

    def sound_centres(self, record, indices):
        """Per clip the frame its sound window is centred on: the middle index (the integer mean of the two middle ones of an even
        clip), clipped at the record's frame count (video_dataset.py:393-399)."""
        n, centres = self.num_frames, []
        for c in range(self.num_clips):
            clip = indices[c * n:(c + 1) * n]
            centre = (clip[n // 2 - 1] + clip[n // 2]) // 2 if n % 2 == 0 else clip[n // 2]
            centres.append(min(record.num_frames, int(centre)))
        return centres

    def get_data(self, record, indices):
        """Visual modalities: [(path below root_path, file bytes), ...].  Sound: (windows [num_clips, L] float32, missing [num_clips]
        bool) -- the track is read once; a missing track gives zero windows with their flags set."""
        if self.modality != 'sound':
            out = []
            for name in self.file_names(record, indices):
                with open(os.path.join(self.root_path, name), 'rb') as f:
                    out.append((name, f.read()))
            return out
        centres = self.sound_centres(record, indices)
        need = int(round(self.resampling_rate * self.audio_length))
        path = os.path.join(self.root_path, record.path)
        if not os.path.exists(path):
            return np.zeros((len(centres), need), np.float32), np.ones(len(centres), bool)
        track = read_wav(path)
        windows = [audio.sound_window(track, c, record.start_frame, self.fps, self.audio_length, self.resampling_rate) for c in centres]
        return np.stack(windows), np.zeros(len(centres), bool)

    def get_label(self, record):
        if self.test_mode:
            return record.video_id
        if not self.multi_label:
            return int(record.label)
        label = torch.zeros(self.num_classes, dtype=torch.float)
        for x in record.label:
            label[int(x)] = 1.0
        return label

    def load(self, record, indices):
        """One modality of an item: the files' bytes and the Geometry drawn for them, or the sound windows and their flags."""
        data = self.get_data(record, indices)
        if self.modality == 'sound':
            return dict(modality='sound', wave=data[0], missing=data[1])
        width, height = _frame_size(data[0][1], os.path.join(self.root_path, data[0][0]))
        return dict(modality=self.modality, names=[n for n, _ in data], files=[b for _, b in data],
                    geometry=self.augmentor.sample(width, height))

    def __getitem__(self, index):
        record = self.video_list[index]
        indices = self._sample_indices(record) if self.is_train else self._get_val_indices(record)
        return dict(index=index, indices=indices, data=[self.load(record, indices)], label=self.get_label(record))

    def __len__(self):
        return len(self.video_list)


class MultiVideoDataSet(torch.utils.data.Dataset):
    """Several modalities of the same videos (video_dataset.py:431-522): root_path, modality and augmentor are lists, one entry per
    modality; every root has its own copy of list_file, line for line the same videos.  The indices of an item are drawn once, from
    the first modality's record and the largest num_consecutive_frames, and shared; the label is the first modality's.  Then every
    modality, in order, reads its files and draws its own augmentation."""

    def __init__(self, root_path, list_file, num_groups=64, frames_per_group=1, num_clips=1, modality=('rgb',), dense_sampling=False,
                 fixed_offset=True, image_tmpl='{:05d}.jpg', augmentor=None, is_train=True, test_mode=False, separator=' ',
                 filter_video=0, num_classes=None, fps=29.97, audio_length=1.28, resampling_rate=24000, log=None):
        modality = list(modality)
        augmentor = list(augmentor) if augmentor is not None else [None] * len(modality)
        if not (len(root_path) == len(modality) == len(augmentor)):
            raise ValueError("MultiVideoDataSet: %d roots and %d augmentors for %d modalities" % (len(root_path), len(augmentor), len(modality)))
        self.video_datasets = [VideoDataSet(root_path[i], list_file, num_groups, frames_per_group, num_clips, modality[i], dense_sampling,
                                            fixed_offset, image_tmpl, augmentor[i], is_train, test_mode, separator, filter_video,
                                            num_classes, fps, audio_length, resampling_rate, log) for i in range(len(modality))]
        self.is_train, self.test_mode = is_train, test_mode
        self.num_frames, self.sample_freq = num_groups, frames_per_group
        self.dense_sampling, self.num_clips, self.fixed_offset = dense_sampling, num_clips, fixed_offset
        self.modality, self.num_classes = modality, num_classes
        self.video_list = self.video_datasets[0].video_list
        self.multi_label = self.video_datasets[0].multi_label
        for d in self.video_datasets[1:]:
            if len(d) != len(self.video_list):
                raise ValueError("MultiVideoDataSet: %s lists %d videos, %s %d" % (d.list_file, len(d), self.video_datasets[0].list_file,
                                                                                  len(self.video_list)))
        self.num_consecutive_frames = max(d.num_consecutive_frames for d in self.video_datasets)

    def _sample_indices(self, record):
        return sample_train_clip(record.num_frames, self.num_consecutive_frames, self.num_frames, self.sample_freq, self.dense_sampling,
                                 self.num_clips)

    def _get_val_indices(self, record):
        return sample_val_test_clip(record.num_frames, self.num_consecutive_frames, self.num_frames, self.sample_freq, self.dense_sampling,
                                    self.fixed_offset, self.num_clips)

    def __getitem__(self, index):
        record = self.video_list[index]
        indices = self._sample_indices(record) if self.is_train else self._get_val_indices(record)
        data = [d.load(d.video_list[index], indices) for d in self.video_datasets]
        return dict(index=index, indices=indices, data=data, label=self.video_datasets[0].get_label(record))

    def __len__(self):
        return len(self.video_list)


# ---------------------------------------------------------------------------------------------- batches
def _pillow_video(files, names, modality):
    """[H, W, K_in] uint8: PIL.Image.open of every file, stacked along the channel axis."""
    from PIL import Image
    mode, planes = ('L', []) if modality == 'flow' else ('RGB', [])
    for blob, name in zip(files, names):
        with Image.open(io.BytesIO(blob)) as im:
            if im.mode != mode:
                raise ValueError("%s is a mode-%s image, the %s modality stacks mode-%s files" % (name, im.mode, modality, mode))
            a = np.asarray(im)
        planes.append(a[:, :, None] if a.ndim == 2 else a)
    return np.ascontiguousarray(np.concatenate(planes, axis=2))


class Collate:
    """Items of a MultiVideoDataSet -> ([per modality an EncodedFrames / Frames / Waveforms], targets).  Runs in the loader's workers:
    host memory only, nothing pinned (the DataLoader pins through the objects' pin_memory()).  pillow=True decodes every visual
    batch on the host (a `Frames`: the same pixels, four to ten times the bytes over PCIe) instead of only those the GPU decoder refuses."""
    FILES = {'rgb': 1, 'flow': 2 * CONSECUTIVE, 'rgbdiff': CONSECUTIVE + 1}

    def __init__(self, modality, num_clips, groups, pillow=False):
        self.modality, self.num_clips, self.groups, self.pillow = list(modality), int(num_clips), int(groups), bool(pillow)

    def modal_input(self, items, j):
        """The batch of modality j of the items: an EncodedFrames, the Pillow-decoded Frames where the GPU decoder refuses a file, or
        the sound Waveforms."""
        global pillow_fallbacks
        want = self.num_clips * self.groups
        m = self.modality[j]
        parts = [it['data'][j] for it in items]
        if m == 'sound':
            return audio.Waveforms(np.stack([p['wave'] for p in parts]), np.stack([p['missing'] for p in parts]))
        for it, p in zip(items, parts):
            if len(it['indices']) != want or len(p['files']) != want * self.FILES[m]:
                raise ValueError("%s: video %d has %d frame indices (%d files), the model takes num_clips x groups = %d x %d = %d "
                                 "(%d files): uniform sampling ignores num_clips -- the README recipes use --dense_sampling"
                                 % (m, it['index'], len(it['indices']), len(p['files']), self.num_clips, self.groups, want,
                                    want * self.FILES[m]))
        geos = [p['geometry'] for p in parts]
        encoded = None
        if not self.pillow:
            try:
                encoded = video.EncodedFrames([p['files'] for p in parts], geos)
            except jpeg.Unsupported:
                pillow_fallbacks += 1
        return encoded or video.Frames([_pillow_video(p['files'], p['names'], m) for p in parts], geos)

    @staticmethod
    def targets(items):
        labels = [it['label'] for it in items]
        if torch.is_tensor(labels[0]):
            return torch.stack(labels)
        if isinstance(labels[0], str):
            return labels                                    # test_mode: the video ids
        return torch.tensor(labels, dtype=torch.long)

    def __call__(self, items):
        return [self.modal_input(items, j) for j in range(len(self.modality))], self.targets(items)


class UnimodalCollate(Collate):
    """Items of a VideoDataSet -> (EncodedFrames | Frames | Waveforms, targets): the one modality as a single object, as the bare
    backbones take it (train_unimodal.py hands `images` to the model as the loader yields it)."""

    def __init__(self, modality, num_clips, groups, pillow=False):
        super().__init__([modality], num_clips, groups, pillow)

    def __call__(self, items):
        return self.modal_input(items, 0), self.targets(items)


class Loader:
    """A DataLoader with the epoch bookkeeping the launcher leaves to it: every iteration is one epoch -- a DistributedSampler is told
    its number first, and rank 0 reports at its end how many batches Pillow had to decode."""

    def __init__(self, loader, sampler=None, rank=0, log=print):
        self.loader, self.sampler, self.rank, self.log, self.epoch = loader, sampler, rank, log, 0

    def __len__(self):
        return len(self.loader)

    @property
    def dataset(self):
        return self.loader.dataset

    def __iter__(self):
        global pillow_fallbacks
        if self.sampler is not None and hasattr(self.sampler, 'set_epoch'):
            self.sampler.set_epoch(self.epoch)
        self.epoch += 1
        # the workers' counters stay in their processes: count the Frames that arrive instead (unless they were asked for)
        in_workers = self.loader.num_workers > 0 and not getattr(self.loader.collate_fn, 'pillow', False)
        for inputs, target in self.loader:
            if in_workers:
                pillow_fallbacks += sum(isinstance(x, video.Frames) for x in (inputs if isinstance(inputs, list) else [inputs]))
            yield inputs, target
        if self.rank == 0 and self.log is not None:
            self.log("data: %d batches so far held a JPEG file the GPU decoder does not take and were decoded with Pillow" % pillow_fallbacks)


def loaders(args, rank, world, device):
    """(train_loader, val_loader) for `--loader_factory adamml_amd.data:loaders`: --datadir holds one root per modality (or one root
    for all), each with the dataset's list files."""
    if not args.datadir:
        raise SystemExit("adamml_amd.data:loaders needs --datadir (one root per modality)")
    modality = list(args.modality)
    roots = list(args.datadir) * len(modality) if len(args.datadir) == 1 else list(args.datadir)
    if len(roots) != len(modality):
        raise SystemExit("--datadir takes one path per modality (%d given for %d modalities)" % (len(args.datadir), len(modality)))
    cfg = DATASETS.get(args.dataset, DATASETS['kinetics-sounds'])
    device = torch.device(device)
    batch = max(1, args.batch_size // world)
    workers = min(args.workers, len(os.sched_getaffinity(0)))
    log = print if rank == 0 else None
    out = []
    for is_train, list_file, num_clips in ((True, cfg['train_list'], args.num_segments), (False, cfg['val_list'], args.val_num_clips)):
        augs = [None if m == 'sound' else video.augmentor_for(args, m, is_train) for m in modality]
        ds = MultiVideoDataSet(roots, list_file, args.groups, args.frames_per_group, num_clips=num_clips, modality=modality,
                               dense_sampling=args.dense_sampling, image_tmpl=cfg['image_tmpl'], augmentor=augs, is_train=is_train,
                               separator=cfg['separator'], filter_video=cfg['filter_video'], num_classes=args.num_classes, fps=args.fps,
                               audio_length=args.audio_length, resampling_rate=args.resampling_rate, log=log)
        sampler = None
        if world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=is_train)
        dl = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=is_train and sampler is None, sampler=sampler, num_workers=workers,
                                         collate_fn=Collate(modality, num_clips, args.groups), pin_memory=device.type == 'cuda')
        out.append(Loader(dl, sampler, rank, log))
    return tuple(out)


def unimodal_loaders(args, rank, world, device):
    """(train_loader, val_loader) of train_unimodal.py:207-256 for `--loader_factory adamml_amd.data:unimodal_loaders` (the unimodal
    launcher's default with --datadir): ONE modality below ONE root, args.num_clips clips per video in both loaders, and batches
    whose first element is the modality's object itself, not a list."""
    modality = args.modality if isinstance(args.modality, str) else args.modality[0]
    root = args.datadir if isinstance(args.datadir, str) or not args.datadir else args.datadir[0]
    if not root:
        raise SystemExit("adamml_amd.data:unimodal_loaders needs --datadir (the root of the one modality)")
    cfg = DATASETS.get(args.dataset, DATASETS['kinetics-sounds'])
    device = torch.device(device)
    batch = max(1, int(args.batch_size / world))
    workers = min(args.workers, len(os.sched_getaffinity(0)))
    log = print if rank == 0 else None
    out = []
    for is_train, list_file in ((True, cfg['train_list']), (False, cfg['val_list'])):
        aug = None if modality == 'sound' else video.augmentor_for(args, modality, is_train)
        ds = VideoDataSet(root, list_file, args.groups, args.frames_per_group, num_clips=args.num_clips, modality=modality,
                          dense_sampling=args.dense_sampling, image_tmpl=cfg['image_tmpl'], augmentor=aug, is_train=is_train,
                          separator=cfg['separator'], filter_video=cfg['filter_video'], num_classes=args.num_classes, fps=args.fps,
                          audio_length=args.audio_length, resampling_rate=args.resampling_rate, log=log)
        sampler = None
        if world > 1:
            sampler = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=is_train)
        dl = torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=is_train and sampler is None, sampler=sampler, num_workers=workers,
                                         collate_fn=UnimodalCollate(modality, args.num_clips, args.groups), pin_memory=device.type == 'cuda')
        out.append(Loader(dl, sampler, rank, log))
    return tuple(out)
