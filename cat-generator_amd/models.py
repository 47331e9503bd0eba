"""models.lua's generator / discriminator factories, translated line for line onto the engine's nn layer.

Only the definitions the front ends reach are here: G32up-c (models.lua:196-228, the default
via create_G :234-240), G32up (:138-160) and its 16x16 form G16up (:108-132, what create_G returns at --scale 16),
D32_st3 (:640-711, the only D create_D returns, :276; it builds at 16, 32 and 64 px) and the
spatial-transformer factory (:814-906), the validator V (:716-804) that train_v.py trains, and G's encoder / auto-encoder form
(:50-83, :246-262) that pretrain_g.py trains.  `create_G32up_c_64` is the builder-defined 64x64 extension of
BASELINE.json config #5.
"""
from . import cudnn, nn
from .tensor import Tensor
from .weight_init import w_init


def create_G_decoder_upsampling32(dimensions, noiseDim, base=8):
    """models.lua:138-160.  `base` is the side of the first map: 8 in the reference (8x8 -> 32x32); base=4 is models.lua:108-132."""
    model = nn.Sequential()
    model.add(nn.Linear(noiseDim, 128 * base * base))
    model.add(nn.View(128, base, base))
    model.add(nn.PReLU(None, None, True))

    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(128, 256, 5, 5, 1, 1, (5 - 1) // 2, (5 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(256))
    model.add(nn.PReLU(None, None, True))

    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(256, 128, 5, 5, 1, 1, (5 - 1) // 2, (5 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(128))
    model.add(nn.PReLU(None, None, True))

    model.add(cudnn.SpatialConvolution(128, dimensions[0], 3, 3, 1, 1, (3 - 1) // 2, (3 - 1) // 2))
    model.add(nn.Sigmoid())

    model = w_init(model, "heuristic")
    return model


def create_G_decoder_upsampling16(dimensions, noiseDim):
    """models.lua:108-132 (G16up): create_G_decoder_upsampling32 from a 4x4 map, 4x4 -> 8x8 -> 16x16."""
    return create_G_decoder_upsampling32(dimensions, noiseDim, base=4)


def create_G_decoder_upsampling32c(dimensions, noiseDim, base=4):
    """models.lua:196-228.  `base` is 4 in the reference (4x4 -> 32x32); base=8 gives the 64x64 extension."""
    model = nn.Sequential()
    # 4x4
    model.add(nn.Linear(noiseDim, 512 * base * base))
    model.add(nn.PReLU(None, None, True))
    model.add(nn.View(512, base, base))

    # 4x4 -> 8x8
    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(512, 512, 3, 3, 1, 1, (3 - 1) // 2, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(512))
    model.add(nn.PReLU(None, None, True))

    # 8x8 -> 16x16
    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(512, 256, 3, 3, 1, 1, (3 - 1) // 2, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(256))
    model.add(nn.PReLU(None, None, True))

    # 16x16 -> 32x32
    model.add(nn.SpatialUpSamplingNearest(2))
    model.add(cudnn.SpatialConvolution(256, 128, 5, 5, 1, 1, (5 - 1) // 2, (5 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(128))
    model.add(nn.PReLU(None, None, True))

    model.add(cudnn.SpatialConvolution(128, dimensions[0], 3, 3, 1, 1, (3 - 1) // 2, (3 - 1) // 2))
    model.add(nn.Sigmoid())

    model = w_init(model, "heuristic")
    return model


def create_G32up_c_64(dimensions, noiseDim):
    """BASELINE.json config #5: G32up-c scaled to 64x64 (first Linear -> 512*8*8)."""
    return create_G_decoder_upsampling32c(dimensions, noiseDim, base=8)


def create_G(dimensions, noiseDim):
    """models.lua:234-240: G16up at 16 px, G32up-c otherwise (and its 64x64 extension)."""
    if dimensions[1] == 16:
        return create_G_decoder_upsampling16(dimensions, noiseDim)
    if dimensions[1] == 64:
        return create_G32up_c_64(dimensions, noiseDim)
    return create_G_decoder_upsampling32c(dimensions, noiseDim)


def create_G_encoder32(dimensions, noiseDim):
    """models.lua:50-83: the encoder half of G in auto-encoder form (pretrain_g.lua).  Three 2x2 poolings: the flattened map has
    32 * H/8 * W/8 features (32 * 0.25^3 * H * W, :73-74), which is what makes the same definition serve 64x64."""
    model = nn.Sequential()
    activation = nn.LeakyReLU

    model.add(nn.SpatialConvolution(dimensions[0], 16, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(16))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))

    model.add(nn.SpatialConvolution(16, 16, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(16))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))

    model.add(nn.SpatialConvolution(16, 32, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(32))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))

    model.add(nn.SpatialConvolution(32, 32, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(32))
    model.add(activation())

    feat = 32 * dimensions[1] * dimensions[2] // (4 * 4 * 4)
    model.add(nn.View(feat))
    model.add(nn.Linear(feat, 1024))
    model.add(nn.BatchNormalization(1024))
    model.add(activation())
    model.add(nn.Linear(1024, noiseDim))

    model = w_init(model, "heuristic")
    return model


def create_G_autoencoder(dimensions, noiseDim):
    """models.lua:246-262: nn.Sequential{encoder, decoder}.  The decoder is what create_G returns for these dimensions (G32up-c, its
    64x64 extension when dimensions[1] == 64), so the half pretrain_g.py saves is the net train.py trains.  At 16 px the reference
    pairs create_G_encoder16 with G16up (:248-250); that encoder is not written here (pre-training is the optional step, and
    tests/test_pretrain_host.py pins this refusal), so 16 px raises.  The tree holds modules
    the planned executor has no entry for (nn.BatchNormalization): it runs on the per-module walk, encoder and decoder alike."""
    model = nn.Sequential()
    if dimensions[1] == 16:
        raise NotImplementedError("create_G_encoder16 (models.lua:14) is not implemented: G can be trained and sampled at 16 px "
                                  "(create_G), but not pre-trained as an auto-encoder")
    model.add(create_G_encoder32(dimensions, noiseDim))
    model.add(create_G(dimensions, noiseDim))
    return model


def create_D(dimensions, cuda=False):
    """models.lua:268-277: always st3."""
    return create_D32_st3(dimensions, cuda)


def create_D32_st3(dimensions, cuda=False):
    """models.lua:640-711.  `cuda` only decides whether the nn.Copy host<->device layers wrap the net
    (:642-644, :703-706); the arithmetic always runs on the device."""
    conv = nn.Sequential()
    if cuda:
        conv.add(nn.Copy("torch.FloatTensor", "torch.CudaTensor", True, True))
    conv.add(createSpatialTransformer(True, False, False, dimensions[1], dimensions[0], cuda))
    conv.add(nn.SpatialConvolution(dimensions[0], 64, 3, 3, 1, 1, (3 - 1) // 2))
    conv.add(nn.PReLU(None, None, True))
    conv.add(nn.SpatialConvolution(64, 64, 3, 3, 1, 1, (3 - 1) // 2))
    conv.add(nn.PReLU(None, None, True))
    conv.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    conv.add(nn.SpatialDropout(0.2))

    def st_branch():
        b = nn.Sequential()
        b.add(createSpatialTransformer(True, True, True, dimensions[1] // 2, 64, cuda))
        b.add(nn.SpatialConvolution(64, 64, 3, 3, 1, 1, (3 - 1) // 2))
        b.add(nn.PReLU(None, None, True))
        b.add(nn.SpatialMaxPooling(2, 2))
        b.add(nn.SpatialDropout(0.2))
        b.add(nn.SpatialConvolution(64, 64, 3, 3, 1, 1, (3 - 1) // 2))
        b.add(nn.PReLU(None, None, True))
        return b

    branch1 = st_branch()
    branch2 = st_branch()
    branch3 = st_branch()

    branch4 = nn.Sequential()
    branch4.add(nn.SpatialConvolution(64, 128, 5, 5, 1, 1, (5 - 1) // 2))
    branch4.add(nn.PReLU(None, None, True))
    branch4.add(nn.SpatialMaxPooling(2, 2))
    branch4.add(nn.SpatialDropout(0.2))
    branch4.add(nn.SpatialConvolution(128, 128, 7, 7, 1, 1, (7 - 1) // 2))
    branch4.add(nn.PReLU(None, None, True))

    concy = nn.Concat(2)
    concy.add(branch1)
    concy.add(branch2)
    concy.add(branch3)
    concy.add(branch4)

    conv.add(concy)
    conv.add(nn.SpatialDropout())
    feat = (64 + 64 + 64 + 128) * (dimensions[1] // 4) * (dimensions[2] // 4)
    conv.add(nn.View(feat))
    conv.add(nn.Linear(feat, 256))
    conv.add(nn.PReLU(None, None, True))
    conv.add(nn.Dropout())
    conv.add(nn.Linear(256, 1))
    conv.add(nn.Sigmoid())

    if cuda:
        conv.add(nn.Copy("torch.CudaTensor", "torch.FloatTensor", True, True))
        conv.cuda()

    conv = w_init(conv, "heuristic")
    return conv


def create_V(dimensions):
    """models.lua:716-722."""
    if dimensions[1] == 16:
        return create_V16(dimensions)
    return create_V32(dimensions)


def _v_head(model, feat):
    """models.lua:742-754 / :790-802: two Linear -> BatchNormalization -> LeakyReLU -> Dropout blocks and a 2-way SoftMax."""
    activation = nn.LeakyReLU
    model.add(nn.View(feat))
    model.add(nn.Linear(feat, 1024))
    model.add(nn.BatchNormalization(1024))
    model.add(activation())
    model.add(nn.Dropout())

    model.add(nn.Linear(1024, 1024))
    model.add(nn.BatchNormalization(1024))
    model.add(activation())
    model.add(nn.Dropout())

    model.add(nn.Linear(1024, 2))
    model.add(nn.SoftMax())
    return w_init(model, "heuristic")


def create_V16(dimensions):
    """models.lua:724-759."""
    model = nn.Sequential()
    activation = nn.LeakyReLU

    model.add(nn.SpatialConvolution(dimensions[0], 128, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(activation())
    model.add(nn.SpatialConvolution(128, 128, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(128))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))
    model.add(nn.SpatialDropout(0.2))

    model.add(nn.SpatialConvolution(128, 256, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(activation())
    model.add(nn.SpatialConvolution(256, 256, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(256))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))
    model.add(nn.SpatialDropout())

    imgSize = dimensions[1] * dimensions[2] // (4 * 4)
    return _v_head(model, 256 * imgSize)


def create_V32(dimensions):
    """models.lua:761-804 (the nn.Dropout at :776 acts on a 4-D map: an element-wise mask)."""
    model = nn.Sequential()
    activation = nn.LeakyReLU

    model.add(nn.SpatialConvolution(dimensions[0], 128, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))
    model.add(nn.SpatialConvolution(128, 128, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(128))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))
    model.add(nn.Dropout())

    model.add(nn.SpatialConvolution(128, 256, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(activation())
    model.add(nn.SpatialConvolution(256, 256, 3, 3, 1, 1, (3 - 1) // 2))
    model.add(nn.SpatialBatchNormalization(256))
    model.add(activation())
    model.add(nn.SpatialMaxPooling(2, 2))
    model.add(nn.SpatialDropout())

    imgSize = dimensions[1] * dimensions[2] // (8 * 8)
    return _v_head(model, 256 * imgSize)


def createSpatialTransformer(allow_rotation, allow_scaling, allow_translation, input_size, input_channels, cuda=True):
    """models.lua:814-906.  The reference forces the sampler onto the CPU in GPU mode (:889-899) and wraps it in
    nn.Copy layers; the engine's sampler is a device kernel, so those copies (pure transport) are not added."""
    init_bias = []
    nbr_params = 0
    if allow_rotation:
        nbr_params += 1
        init_bias.append(0)
    if allow_scaling:
        nbr_params += 1
        init_bias.append(1)
    if allow_translation:
        nbr_params += 2
        init_bias += [0, 0]
    if nbr_params == 0:
        raise NotImplementedError("fully parametrised transformer (6 params) is not used by create_D32_st3")

    # localization network
    net = nn.Sequential()
    net.add(nn.SpatialAveragePooling(2, 2, 2, 2))
    net.add(nn.SpatialConvolution(input_channels, 16, 3, 3, 1, 1, (3 - 1) // 2))
    net.add(nn.LeakyReLU())
    net.add(nn.SpatialConvolution(16, 16, 3, 3, 1, 1, (3 - 1) // 2))
    net.add(nn.LeakyReLU())
    net.add(nn.SpatialAveragePooling(2, 2, 2, 2))

    newHeight = input_size // 4
    net.add(nn.View(16 * newHeight * newHeight))
    net.add(nn.Linear(16 * newHeight * newHeight, 64))
    net.add(nn.LeakyReLU())
    classifier = nn.Linear(64, nbr_params)
    net.add(classifier)

    net = w_init(net, "heuristic")
    # identity initialisation (see paper, A.3 section): models.lua:859-860
    classifier.weight.zero()
    classifier.bias = Tensor.from_numpy(init_bias)  # replaces the tensor object, as the reference does

    localization_network = net

    ct = nn.ConcatTable()
    branch1 = nn.Sequential()
    branch1.add(nn.Transpose((3, 4), (2, 4)))
    branch2 = nn.Sequential()
    branch2.add(localization_network)
    branch2.add(nn.AffineTransformMatrixGenerator(allow_rotation, allow_scaling, allow_translation))
    branch2.add(nn.AffineGridGeneratorBHWD(input_size, input_size))
    ct.add(branch1)
    ct.add(branch2)

    st = nn.Sequential()
    st.add(ct)
    sampler = nn.BilinearSamplerBHWD()
    st.add(sampler)
    st.add(nn.Transpose((2, 4), (3, 4)))
    return st
