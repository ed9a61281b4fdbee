"""Mid-stream control changes in the COMPILED reference (test infrastructure, the oracle of solo_batch_update_streams).

The reference's public header has no setter, but its core takes the control on every call: AGR_Sate_Encoder_Encode hands
SATEEncCtl.encControl to SKP_Silk_SDK_Encode for every 20 ms frame, which reads bitRate, useDTX and useMDIndex each time
(SKP_Silk_enc_API.c:165-176; setup_rate_FIX re-derives the SNR targets when the rate moved), and SKP_Silk_SDK_Decode takes
decControl.useMDIndex on every call (SKP_Silk_dec_API.c:107).  So a value written into the handle between two packets applies from the
next packet on -- what a setter would do.  The handle is the malloc'ed SATEEncCtl / SATEDecCtl (libBWE/AGR_BWE_structs.h:61-76); on LP64,
after its two leading pointers:

  SATEEncCtl.encControl (SKP_SILK_SDK_EncControlStruct) at 16: API_sampleRate +0, bitRate +12, useDTX +28, useMDIndex +32
  SATEDecCtl.decControl (SKP_SILK_SDK_DecControlStruct) at 16: API_sampleRate +0, framesPerPacket +8, useMDIndex +20

The offsets are checked against what Init wrote before anything is poked, so a layout that differs fails loudly instead of writing
elsewhere.  bitRate is the SILK rate: targetRate_bps (<= 0 meaning 15600, AGR_BWE_SDK_API.c:35) minus the high-band share, 1600, or 800
with joint_mode 1 (AGR_BWE_SDK_API.c:119)."""
import ctypes as C

import refcodec as R

ENC_API_FS, ENC_BITRATE, ENC_DTX, ENC_MDI = 16, 28, 44, 48
DEC_API_FS, DEC_FPP, DEC_MDI = 16, 24, 36


def silk_rate(target_bps, joint=0):
    """the bitRate AGR_Sate_Encoder_Init stores for a targetRate_bps"""
    t = 15600 if target_bps <= 0 else target_bps
    return t - (800 if joint else 1600)


def _word(h, off):
    return C.c_int32.from_address(h + off)


def _expect(h, off, want, what):
    got = _word(h, off).value
    if got != want:
        raise AssertionError("reference handle layout: %s at offset %d is %d, Init wrote %d" % (what, off, got, want))


class PokeEncoder(R.RefEncoder):
    """a compiled-reference encoder whose rate, DTX and useMDIndex can change between two packets"""

    def __init__(self, kind="fix", rate=13600, joint=0, dtx=0, samplerate=16000, use_md_index=0, framesize_ms=40):
        super().__init__(kind, rate=rate, joint=joint, dtx=dtx, samplerate=samplerate, use_md_index=use_md_index, framesize_ms=framesize_ms)
        self.joint = joint
        _expect(self.h, ENC_API_FS, 16000 if samplerate == 32000 else 8000, "encControl.API_sampleRate")
        _expect(self.h, ENC_BITRATE, silk_rate(rate, joint), "encControl.bitRate")
        _expect(self.h, ENC_DTX, 1 if dtx else 0, "encControl.useDTX")
        _expect(self.h, ENC_MDI, use_md_index, "encControl.useMDIndex")

    def control(self):
        """(SILK rate, useDTX, useMDIndex) as the handle holds them"""
        return tuple(_word(self.h, o).value for o in (ENC_BITRATE, ENC_DTX, ENC_MDI))

    def set_control(self, rate=None, dtx=None, use_md_index=None):
        """rate: targetRate_bps (the SILK rate is derived as Init does); None leaves a field as it is"""
        if rate is not None:
            _word(self.h, ENC_BITRATE).value = silk_rate(int(rate), self.joint)
        if dtx is not None:
            _word(self.h, ENC_DTX).value = 1 if dtx else 0
        if use_md_index is not None:
            _word(self.h, ENC_MDI).value = int(use_md_index)


class PokeDecoder(R.RefDecoder):
    """a compiled-reference decoder whose useMDIndex can change between two packets"""

    def __init__(self, kind="fix", joint=0, samplerate=16000, use_md_index=0, framesize_ms=40):
        super().__init__(kind, joint=joint, samplerate=samplerate, use_md_index=use_md_index, framesize_ms=framesize_ms)
        _expect(self.h, DEC_API_FS, 16000 if samplerate == 32000 else 8000, "decControl.API_sampleRate")
        _expect(self.h, DEC_FPP, 1, "decControl.framesPerPacket")
        _expect(self.h, DEC_MDI, use_md_index, "decControl.useMDIndex")

    def set_control(self, use_md_index=None):
        if use_md_index is not None:
            _word(self.h, DEC_MDI).value = int(use_md_index)
