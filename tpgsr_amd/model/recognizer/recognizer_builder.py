"""RecognizerBuilder (reference: model/recognizer/recognizer_builder.py:27-104): the integrated ASTER recognizer.  Evaluation path with
rectification (bilinear down-sample to 32x64 -> STN head -> TPS to 32x100), encoder, then AttentionRecognitionHead.sample (greedy, the
default) or, with beam_width >= 1, AttentionRecognitionHead.beam_search: the decode the reference evaluates with (its beam_width is 5,
recognizer_builder.py:24, :93)."""
import torch
from torch import nn

from ... import functional as Fh
from ..tps_spatial_transformer import TPSSpatialTransformer
from .attention_recognition_head import MAX_BEAM_WIDTH, AttentionRecognitionHead
from .resnet_aster import ResNet_ASTER
from .stn_head import STNHead

tps_inputsize = [32, 64]
tps_outputsize = [32, 100]
num_control_points = 20
tps_margins = [0.05, 0.05]


class RecognizerBuilder(nn.Module):
    def __init__(self, arch, rec_num_classes, sDim=512, attDim=512, max_len_labels=100, eos="EOS", STN_ON=True, beam_width=0):
        super().__init__()
        if isinstance(beam_width, bool) or not isinstance(beam_width, int) or not 0 <= beam_width <= MAX_BEAM_WIDTH:
            raise ValueError(f"RecognizerBuilder: beam_width must be 0 (greedy decode) or an integer in 1..{MAX_BEAM_WIDTH} (got {beam_width!r})")
        if beam_width >= 1 and (isinstance(eos, bool) or not isinstance(eos, int)):
            raise ValueError(f"RecognizerBuilder: the beam-search decode needs the integer class id of the end-of-sequence symbol, "
                             f"eos=voc.index(\"EOS\") (got eos={eos!r})")
        self.beam_width = beam_width
        self.arch, self.rec_num_classes, self.sDim, self.attDim = arch, rec_num_classes, sDim, attDim
        self.max_len_labels, self.eos, self.STN_ON = max_len_labels, eos, STN_ON
        self.tps_inputsize = tps_inputsize
        self.encoder = ResNet_ASTER(self.arch)
        self.decoder = AttentionRecognitionHead(num_classes=rec_num_classes, in_planes=self.encoder.out_planes, sDim=sDim, attDim=attDim,
                                                max_len_labels=max_len_labels)
        if self.STN_ON:
            self.tps = TPSSpatialTransformer(output_image_size=tuple(tps_outputsize), num_control_points=num_control_points,
                                             margins=tuple(tps_margins))
            self.stn_head = STNHead(in_planes=3, num_ctrlpoints=num_control_points, activation="none")

    def rectify(self, x):
        """(N, 3, H, W) in [-1, 1] -> (rectified (N, 3, 32, 100), control points (N, 20, 2))"""
        stn_in = Fh.to_nchw(Fh.interpolate_bilinear(Fh.to_nhwc(x), tuple(self.tps_inputsize)))
        _, ctrl = self.stn_head(stn_in)
        rect, _ = self.tps(x, ctrl)
        return rect, ctrl

    def forward(self, input_dict):
        """evaluation: {'images': (N, 3, 32, 128) in [-1, 1], ...} -> {'losses': {}, 'output': {'pred_rec', 'pred_rec_score'}} with the
        greedy decode (beam_width = 0) or the reference's beam search (beam_width >= 1: pred_rec_score is all ones, as the reference
        returns it); the reference's loss against dummy targets is not computed"""
        if self.training:
            raise RuntimeError("RecognizerBuilder is an evaluation recognizer here (interfaces/base.py:831-842 loads it frozen); call .eval()")
        x = input_dict["images"] if isinstance(input_dict, dict) else input_dict
        with torch.no_grad():
            out = {"losses": {}, "output": {}}
            if self.STN_ON:
                x, ctrl = self.rectify(x)
                out["output"]["ctrl_points"], out["output"]["rectified_images"] = ctrl, x
            feats = self.encoder(x)
            out["output"]["encoder_feats"] = feats
            if self.beam_width >= 1:
                ids, scores = self.decoder.beam_search(feats, self.beam_width, self.eos)
            else:
                ids, scores = self.decoder.sample([feats, None, None])
            out["output"]["pred_rec"], out["output"]["pred_rec_score"] = ids, scores
            return out
