"""``Sal360Dataset`` of /root/reference/data/dataset.py:13-83: windows of ``seq_len`` consecutive static-model features
(``<video_dir>/<category>/cube_feat/{:06}.npy``) and optical flows (``<motion_dir>/<category>/motion/{:06}.npy``) of the
categories listed in ``input_d_list``.  A window starts at every file whose number is < max_len - seq_len + 1 (max_len = the
highest file number of the category).  Items are (seq, motion, category, filename): lists of seq_len f32 tensors.
numpy file I/O only (the reference's cv2 / torchvision / PIL imports are unused)."""
import os

import numpy as np
import torch


class Sal360Dataset:
    def __init__(self, video_dir, motion_dir, input_d_list, seq_len, transform=None):
        self.video_dir = video_dir
        self.motion_dir = motion_dir
        self.seq_len = seq_len
        with open(input_d_list, "r") as ffile:
            self.data_list = [x.split('\n')[0] for x in ffile.readlines()]
        self.data = []
        self.motion = []
        video_categories = sorted(os.listdir(video_dir))
        for video_category in video_categories:
            if video_category not in self.data_list:
                continue
            print("Got {}".format(video_category))
            feat_sequences = sorted(os.listdir(os.path.join(self.video_dir, video_category, 'cube_feat')))
            max_len = int(feat_sequences[-1].split('.')[0])
            for seq in feat_sequences:
                if ('.npy' in seq) and int(seq.split('.')[0]) < (max_len - seq_len + 1):
                    self.data.append(os.path.join(self.video_dir, video_category, 'cube_feat', seq))
            motion_sequences = sorted(os.listdir(os.path.join(self.motion_dir, video_category, 'motion')))
            for seq in motion_sequences:
                if ('.npy' in seq) and int(seq.split('.')[0]) < (max_len - seq_len + 1):
                    self.motion.append(os.path.join(self.motion_dir, video_category, 'motion', seq))
        assert len(self.data) == len(self.motion)
        self.transform = transform

    @staticmethod
    def _offset_path(path, offset):
        category, mid_filename, filename = path.split('/')[-3:]
        return os.path.join(path.split(mid_filename)[0], mid_filename,
                            '{:06}{}'.format(int(filename.split('.')[0]) + offset, filename[-4:]))

    def __getitem__(self, index):
        seq = []
        motion = []
        category = self.data[index].split('/')[-3]
        filename = self.data[index].split('/')[-1]
        for offset in range(self.seq_len):
            targ_feat_path = self._offset_path(self.data[index], offset)             # static model features
            if os.path.exists(targ_feat_path):
                seq.append(torch.from_numpy(np.load(targ_feat_path).astype(np.float32)))
            else:
                print("{} doesn't exist.".format(targ_feat_path))
            targ_motion_path = self._offset_path(self.motion[index], offset)         # optical flow
            if os.path.exists(targ_motion_path):
                motion.append(torch.from_numpy(np.load(targ_motion_path).astype(np.float32)))
            else:
                print("{} doesn't exist.".format(targ_motion_path))
        return seq, motion, category, filename

    def __len__(self):
        return len(self.data)
